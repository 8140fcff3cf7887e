"""pch_cluster_centers_f32 / pch_cluster_merge_f32 on the GPU, through the C ABI, ops, the pipeline switch and the
drop-in's module knob, against the numpy statement of tests/merge_cases.py.  Everything is bit or integer equality
(centres: uint32 views, with every NaN taken as one pattern - which NaN a 0 / 0 gives is the processor's choice)."""
import functools
import re

import numpy as np
import pytest
import torch

import las_bytes
import merge_cases as mc
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

SORTED = "trimesh_sorted"        # extents ascending: the tall axis is the height whichever face the box search picks


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _merge_call(cuda, C, r, labels=None, ws_bytes=None, K=None):
    """pch_cluster_merge_f32 as it stands: (rc, map, nmerged, labels)"""
    L = _lib.lib()
    K = len(C) if K is None else K
    c = _dev(np.asarray(C, dtype=np.float32).reshape(-1, 3), cuda)
    lab = None if labels is None else _dev(labels, cuda)
    cmap = torch.full((max(K, 1),), -7, dtype=torch.int32, device=cuda)
    cnt = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    need = L.pch_cluster_merge_ws_bytes(K) if ws_bytes is None else ws_bytes
    ws = torch.empty((max(int(need), 1),), dtype=torch.uint8, device=cuda)
    rc = L.pch_cluster_merge_f32(c.data_ptr() if c.numel() else 0, K, float(r), 0 if lab is None else lab.data_ptr(),
                                 0 if lab is None else lab.numel(), cmap.data_ptr(), cnt.data_ptr(), ws.data_ptr(),
                                 int(need), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, cmap[:K].cpu().numpy(), int(cnt.item()), None if lab is None else lab.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------ centres
@functools.lru_cache(maxsize=None)
def _centers_case(frame):
    P, lab, K = mc.centers_cloud(frame)
    return P, lab, K, mc.centers(P, lab, K)


@pytest.mark.parametrize("frame", list(mc.FRAMES))
def test_centers_equal_np_mean(cuda, frame):
    P, lab, K, (want, sizes) = _centers_case(frame)
    x = _dev(P, cuda)
    perm, offsets, _ = ops.segment_by_label(_dev(lab, cuda), x, K)
    got, got_sizes = ops.cluster_centers(x, perm, offsets, K)
    assert got.dtype == torch.float32 and got.shape == (K, 3) and got_sizes.dtype == torch.int64
    np.testing.assert_array_equal(got_sizes.cpu().numpy(), sizes)
    g = got.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(g), np.isnan(want))
    np.testing.assert_array_equal(mc.canonical_bits(g), mc.canonical_bits(want))
    assert np.isnan(g[10]).all() and g[12, 2] == np.inf


def test_centers_of_no_cluster_and_of_no_row(cuda):
    x = _dev(np.zeros((0, 3), dtype=np.float32), cuda)
    lab = torch.empty((0,), dtype=torch.int32, device=cuda)
    for K in (0, 3):
        perm, offsets, _ = ops.segment_by_label(lab, x, K)
        c, s = ops.cluster_centers(x, perm, offsets, K)
        assert c.shape == (K, 3) and torch.isnan(c).all() and not s.any()


# ---------------------------------------------------------------------------------------------------------- merge map
def _map_sets():
    for K in mc.KS:
        yield f"uniform{K}", mc.uniform_centers(K), 6.0
        yield f"lattice{K}", mc.lattice_centers(K), 6.0
        yield f"nan_dup{K}", mc.nan_dup_centers(K), 6.0
        yield f"nan_dup{K}_r0", mc.nan_dup_centers(K), 0.0
    yield "chain", mc.chain_centers(1), 6.0
    yield "two_chains", mc.chain_centers(2), 6.0


@pytest.mark.parametrize("name,C,r", [pytest.param(n, C, r, id=n) for n, C, r in _map_sets()])
def test_map_equals_statement(cuda, name, C, r):
    K = len(C)
    labels = mc.labels_for(K, seed=K)
    want, nwant = mc.merge_map(C, r)
    rc, cmap, n, lab = _merge_call(cuda, C, r, labels)
    assert rc == 0
    np.testing.assert_array_equal(cmap, want)
    assert n == nwant and mc.map_is_ordered(cmap)
    np.testing.assert_array_equal(lab, mc.relabel(labels, want))
    rc, cmap, n, _ = _merge_call(cuda, C, r)                             # labels may be NULL: the map alone
    assert rc == 0 and n == nwant
    np.testing.assert_array_equal(cmap, want)
    if name == "chain":
        assert n == 1
    if name == "two_chains":
        assert n == 2


# ------------------------------------------------------------------------------------------------ ops.merge_clusters
@pytest.mark.parametrize("K", [0, 1, 2, 257, 1000])
def test_merge_clusters_regroups(cuda, K):
    P, lab = mc.clustered_cloud(K)
    want = mc.expected(P, lab, K, 6.0)
    x, l = _dev(P, cuda), _dev(lab, cuda)
    perm, offsets, _ = ops.segment_by_label(l, x, K)
    keep = l.clone()
    m = ops.merge_clusters(x, l, perm, offsets, K, 6.0)
    assert torch.equal(l, keep) and m["labels"].data_ptr() != l.data_ptr()
    assert m["nclusters"] == want["nmerged"] and m["nclusters_before"] == K
    np.testing.assert_array_equal(m["labels"].cpu().numpy(), want["labels"])
    np.testing.assert_array_equal(m["map"].cpu().numpy(), want["map"])
    np.testing.assert_array_equal(mc.canonical_bits(m["centers"].cpu().numpy()), mc.canonical_bits(want["centers"]))
    p2, o2, s2 = ops.segment_by_label(_dev(want["labels"], cuda), x, want["nmerged"])
    assert torch.equal(m["perm"], p2) and torch.equal(m["offsets"], o2)
    np.testing.assert_array_equal(m["stats"].cpu().numpy().view(np.uint32), s2.cpu().numpy().view(np.uint32))
    offs, pm = m["offsets"].cpu().numpy(), m["perm"].cpu().numpy()
    for c in range(0, want["nmerged"], 37):
        np.testing.assert_array_equal(pm[offs[c]:offs[c + 1]], np.flatnonzero(want["labels"] == c))


# -------------------------------------------------------------------------------------------------------------- errors
def test_errors(cuda):
    C = mc.uniform_centers(65)
    for bad in (-1.0, float("nan"), float("inf")):
        assert _merge_call(cuda, C, bad)[0] == -1                       # PCH_ERR_ARG
    assert _merge_call(cuda, C[:1], 6.0, K=65_537)[0] == -4             # PCH_ERR_RANGE, before anything is read
    need = _lib.lib().pch_cluster_merge_ws_bytes(65)
    assert _merge_call(cuda, C, 6.0, ws_bytes=need - 1)[0] == -2        # PCH_ERR_WORKSPACE
    with pytest.raises(_lib.PchError, match="PCH_ERR_ARG"):
        P, lab = mc.clustered_cloud(2)
        x, l = _dev(P, cuda), _dev(lab, cuda)
        perm, offsets, _ = ops.segment_by_label(l, x, 2)
        ops.merge_clusters(x, l, perm, offsets, 2, merge_threshold=-6.0)
    rc, cmap, n, lab = _merge_call(cuda, np.zeros((0, 3), dtype=np.float32), 6.0, np.array([-1, 0, 5], dtype=np.int32))
    assert rc == 0 and n == 0 and lab.tolist() == [-1, -1, -1]


# ---------------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _e2e():
    """the statement of the end-to-end case: stage B and the chunked fit by the CPU oracle, the merge by merge_cases"""
    from oracle import dbscan as odb
    from oracle import ground_filter as ogf
    raw, tower = mc.e2e_cloud()
    g = ogf.ground_filter(raw)
    labels = odb.dbscan_chunked(g["filtered"], mc.E2E["eps"], mc.E2E["min_points"], mc.E2E["chunk_size"], fit="sklearn")
    K = int(labels.max()) + 1
    want = mc.expected(g["filtered"], labels, K, 6.0)
    # the conditions on the case, on the statement alone (test_cluster_merge_host.py asserts the rest of them)
    assert K == 6 and want["nmerged"] == 4 and want["map"].tolist() == [0, 1, 1, 2, 3, 3]
    return raw, g, labels, K, want


def _cluster(cuda, **kw):
    raw = _e2e()[0]
    return pipeline.cluster_points(_dev(raw, cuda), mc.E2E["eps"], mc.E2E["min_points"], mc.E2E["chunk_size"], **kw)


def test_pipeline_switch_equals_statement(cuda):
    raw, g, labels, K, want = _e2e()
    plain = _cluster(cuda)
    assert plain["nclusters"] == K and "merge" not in plain
    np.testing.assert_array_equal(plain["labels"].cpu().numpy(), labels)
    cl = _cluster(cuda, merge_threshold=6.0)
    assert cl["nclusters"] == 4 and cl["merge"]["nclusters_before"] == K
    np.testing.assert_array_equal(cl["labels"].cpu().numpy(), want["labels"])
    np.testing.assert_array_equal(cl["merge"]["map"].cpu().numpy(), want["map"])
    np.testing.assert_array_equal(mc.canonical_bits(cl["merge"]["centers"].cpu().numpy()),
                                  mc.canonical_bits(want["centers"]))
    perm, offs = cl["perm"].cpu().numpy(), cl["offsets"].cpu().numpy()
    assert len(offs) == 5 and cl["stats"].shape == (4, 8)
    for c in range(4):
        np.testing.assert_array_equal(perm[offs[c]:offs[c + 1]], np.flatnonzero(want["labels"] == c))
    # every ground mode takes the switch; without the grouping only the labels come back
    nos = _cluster(cuda, merge_threshold=6.0, segment=False)
    assert "perm" not in nos and "offsets" not in nos and nos["nclusters"] == 4
    assert torch.equal(nos["labels"], cl["labels"])
    for mode in ("plane", "plane_tiles"):
        a, b = _cluster(cuda, ground=mode), _cluster(cuda, ground=mode, merge_threshold=6.0)
        pts, lab = a["ground"]["points"].cpu().numpy(), a["labels"].cpu().numpy()
        w = mc.expected(pts, lab, a["nclusters"], 6.0)
        assert b["nclusters"] == w["nmerged"] <= a["nclusters"]
        np.testing.assert_array_equal(b["labels"].cpu().numpy(), w["labels"])
    # a threshold that links nothing leaves the fit as it is
    same = _cluster(cuda, merge_threshold=0.0)
    assert same["nclusters"] == K and torch.equal(same["labels"], plain["labels"]) and torch.equal(same["perm"], plain["perm"])


def test_tower_table_sees_whole_towers(cuda):
    """with the merge every tower comes back with all its clustered rows; without it the towers cut by a chunk
    boundary come back with their first piece's rows - today's behaviour"""
    raw, g, labels, K, want = _e2e()
    full = np.bincount(want["labels"][want["labels"] >= 0]).tolist()
    towers = pipeline.tower_table(_cluster(cuda, merge_threshold=6.0), extent_order=SORTED)
    assert [t["label"] for t in towers] == [0, 1, 2, 3]
    assert [len(t["points"]) for t in towers] == full == [1200, 1600, 1000, 1400]
    for t in towers:
        np.testing.assert_array_equal(t["points"].view(np.uint32), g["filtered"][want["labels"] == t["label"]].view(np.uint32))
    logs = []
    pieces = pipeline.tower_table(_cluster(cuda), extent_order=SORTED, log=logs.append)
    assert [t["label"] for t in pieces] == [0, 1, 3, 4] and sum("跳过重复杆塔" in m for m in logs) == 2
    assert [len(t["points"]) for t in pieces] == [1200, 800, 1000, 200]


# ------------------------------------------------------------------------------------------------------------- drop-in
def test_drop_in_knob(cuda, tmp_path, monkeypatch):
    from oracle import voxel as ovx
    from pointcloudhookup_amd.utils import tower_extraction as te
    raw = _e2e()[0]
    scales, offsets = np.array([0.001, 0.001, 0.001]), np.array([437000.0, 3139000.0, 0.0])
    XYZ = np.round((raw.astype(np.float64) - offsets) / scales).astype(np.int32)
    path = str(tmp_path / "towers.las")
    las_bytes.build(path, XYZ, scales=scales, offsets=offsets)
    back = np.stack([ovx.las_scaled(XYZ[:, a], scales[a], offsets[a]) for a in range(3)], axis=1).astype(np.float32)
    from oracle import dbscan as odb
    from oracle import ground_filter as ogf
    g = ogf.ground_filter(back)
    labels = odb.dbscan_chunked(g["filtered"], 8.0, 20, 2000, fit="sklearn")
    want = mc.expected(g["filtered"], labels, int(labels.max()) + 1, 6.0)
    assert int(labels.max()) + 1 == 6 and want["nmerged"] == 4          # the case survives the LAS quantisation
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(te, "CHUNK_SIZE", 2000)
    monkeypatch.setattr(te, "OBB_EXTENT_ORDER", SORTED)

    def run():
        logs, prog = [], []
        towers = te.extract_towers(path, progress_callback=prog.append, log_callback=logs.append, min_points=20)
        return towers, logs, prog

    assert te.MERGE_THRESHOLD is None
    off, off_logs, off_prog = run()
    assert not any("合并" in m for m in off_logs) and "\n=== 开始杆塔检测（候选簇：6个） ===" in off_logs
    assert [len(t["points"]) for t in off] == [1200, 800, 1000, 200]
    monkeypatch.setattr(te, "MERGE_THRESHOLD", 6.0)
    on, logs, prog = run()
    at = logs.index("\n=== 合并相邻簇 ===")
    assert logs[at + 1] == "✅ 合并后簇数量: 4" and logs[at + 2] == "\n=== 开始杆塔检测（候选簇：4个） ==="
    assert logs[at - 1].startswith("处理分块 3/3")
    assert [len(t["points"]) for t in on] == [1200, 1600, 1000, 1400]
    # no new milestone: up to the detection the same values, then one per accepted tower (of 4 instead of 6 candidates)
    assert prog[:prog.index(75) + 1] == off_prog[:off_prog.index(75) + 1]
    assert prog[prog.index(75) + 1:] == [75 + int(15 * (k + 1) / 4) for k in range(4)] + [100]
    assert not any(re.search(r"跳过重复杆塔", m) for m in logs)
    # the knob off again (None and 0 alike): log and towers are those of the unmodified path
    for value in (None, 0.0):
        monkeypatch.setattr(te, "MERGE_THRESHOLD", value)
        again, again_logs, again_prog = run()
        assert again_logs == off_logs and again_prog == off_prog and len(again) == len(off)
        for a, b in zip(again, off):
            assert sorted(a) == sorted(b)
            for key in a:
                np.testing.assert_array_equal(np.asarray(a[key]), np.asarray(b[key]))
