"""pch_upright_boxes_f32 on the GPU, through the C ABI, ops, pipeline.tower_table and the drop-in's module knob, against
the numpy statement of tests/upright_cases.py.  Everything is integer or value equality (-0.0 equals +0.0, NaN in the
same places): the rule is minima and maxima of float64 products, so no order and no tolerance enters."""
import functools
import glob
import os

import numpy as np
import pytest
import torch

import las_bytes
import merge_cases as mc
import upright_cases as uc
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

SORTED = "trimesh_sorted"        # exact mode: extents ascending, so that its height is the tall axis on this cloud
SENTINEL = 0xA5


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(P, labels, K, expected records), computed once"""
    if name in uc.FRAMES:
        P, lab, K = uc.centers_cloud(name)
    elif name == "big":
        P, lab, K = uc.big_cloud()
    elif name == "tile_edges":
        P, lab, K = uc.tile_edges_cloud()
    else:
        P, lab, K, _ = uc.rectangles_cloud()
    return P, lab, K, uc.expected(P, lab, K)


# --------------------------------------------------------------------------------------------------------- records
@pytest.mark.parametrize("name", list(uc.FRAMES) + ["big", "tile_edges", "rectangles"])
def test_records_equal_statement(cuda, name):
    P, lab, K, want = _case(name)
    x = _dev(P, cuda)
    perm, offsets, _ = ops.segment_by_label(_dev(lab, cuda), x, K)
    dev_records = ops.upright_boxes(x, perm, offsets, K)
    assert dev_records.dtype == torch.uint8 and dev_records.shape == (K, 72) and dev_records.is_cuda
    got = ops.upright_boxes(x, perm, offsets, K, to_host=True)
    assert got.dtype == uc.RECORD and got.shape == (K,)
    np.testing.assert_array_equal(dev_records.cpu().numpy(), got.view(np.uint8).reshape(K, 72))   # the same call twice
    uc.assert_records_equal(got, want)
    assert not got["reserved"].any()
    if name in uc.FRAMES:
        assert got["status"].tolist() == [0] * 10 + [1, 1, 1] and got["n"].tolist() == mc.CENTER_SIZES + [0, 300, 300]
    if name == "big":
        assert got["n"][100] == 300_001 and got["n"].max(initial=0, where=np.arange(K) != 100) <= 3
    if name == "tile_edges":
        assert got["n"].tolist() == uc.EDGE_SIZES and not got["status"].any()
    if name == "rectangles":
        names = uc.rectangles_cloud()[3]
        assert got["j"][names.index("wrap_89.97")] == uc.T - 1 and got["j0"][names.index("wrap_89.97")] == 0
        assert got["j"][names.index("single_point")] == 0 and got["j"][names.index("on_fine")] == uc.ON_FINE


def test_angle_table_is_numpys_and_kept(cuda):
    t = ops.upright_angle_table(cuda)
    assert t is ops.upright_angle_table(cuda) and t.dtype == torch.float64 and t.shape == (uc.T, 2)
    np.testing.assert_array_equal(t.cpu().numpy(), uc.table())


# ------------------------------------------------------------------------------------------------------ the C call
def _raw_call(cuda, P, lab, K, ws_bytes=None, nclusters=None, cap=None):
    """pch_upright_boxes_f32 as it stands on cells pre-filled with a sentinel: (rc, the bytes of the records)"""
    L = _lib.lib()
    x = _dev(np.asarray(P, dtype=np.float32).reshape(-1, 3), cuda)
    perm, offsets, _ = ops.segment_by_label(_dev(np.asarray(lab, dtype=np.int32), cuda), x, K)
    out = torch.full((max(K, 1), 72), SENTINEL, dtype=torch.uint8, device=cuda)
    n = perm.numel() if cap is None else cap
    k = K if nclusters is None else nclusters
    need = L.pch_upright_boxes_ws_bytes(K, perm.numel()) if ws_bytes is None else ws_bytes
    ws = torch.empty((max(int(need), 1),), dtype=torch.uint8, device=cuda)
    table = ops.upright_angle_table(cuda)
    rc = L.pch_upright_boxes_f32(x.data_ptr() if x.numel() else 0, perm.data_ptr() if perm.numel() else 0,
                                 offsets.data_ptr(), k, n, table.data_ptr(), out.data_ptr(), ws.data_ptr(), int(need),
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


def test_c_call_edges(cuda):
    P, lab, K, want = _case("rectangles")
    none = np.zeros((0, 3), dtype=np.float32), np.zeros((0,), dtype=np.int32)
    # no cluster: success and no work, with zero rows and with a cloud
    for rows, labels in (none, (P, lab)):
        rc, cells = _raw_call(cuda, rows, labels, 0)
        assert rc == 0 and (cells == SENTINEL).all()
    # clusters, but not one row: every record says so
    rc, cells = _raw_call(cuda, *none, 3)
    got = cells.reshape(-1).view(uc.RECORD)
    assert rc == 0 and got["status"].tolist() == [1, 1, 1] and not got["n"].any() and np.isnan(got["zmax"]).all()
    # every cell of every record is written: no sentinel byte is left where the statement's record has another one
    rc, cells = _raw_call(cuda, P, lab, K)
    assert rc == 0
    got = cells.reshape(-1).view(uc.RECORD)
    uc.assert_records_equal(got, want)
    assert not got["reserved"].any()
    for f in uc.RECORD.names:
        assert not (np.ascontiguousarray(got[f]).view(np.uint8) == SENTINEL).all(), f
    need = _lib.lib().pch_upright_boxes_ws_bytes(K, len(lab))
    assert _raw_call(cuda, P, lab, K, ws_bytes=need - 1)[0] == -2       # PCH_ERR_WORKSPACE
    assert _raw_call(cuda, P, lab, K, nclusters=-1)[0] == -1            # PCH_ERR_ARG
    assert _raw_call(cuda, P, lab, K, cap=-1)[0] == -1
    L = _lib.lib()
    host = np.zeros((uc.T, 2))
    out = torch.empty((K, 72), dtype=torch.uint8, device=cuda)
    assert L.pch_upright_boxes_f32(0, 0, 0, K, 0, ops.upright_angle_table(cuda).data_ptr(), out.data_ptr(), 0, 0, 0) == -1
    assert L.pch_upright_boxes_f32(0, 0, 0, K, 0, host.ctypes.data, out.data_ptr(), 0, 0, 0) == -1   # a host table


# ------------------------------------------------------------------------------------------------------ end to end
@functools.lru_cache(maxsize=None)
def _e2e():
    """the statement of the end-to-end case: stage B and the chunked fit by the CPU oracle, the merge by merge_cases, the
    records by upright_cases"""
    from oracle import dbscan as odb
    from oracle import ground_filter as ogf
    raw, tower = mc.e2e_cloud()
    g = ogf.ground_filter(raw)
    labels = odb.dbscan_chunked(g["filtered"], mc.E2E["eps"], mc.E2E["min_points"], mc.E2E["chunk_size"], fit="sklearn")
    K = int(labels.max()) + 1
    want = mc.expected(g["filtered"], labels, K, 6.0)
    assert K == 6 and want["nmerged"] == 4
    return raw, g, want["labels"], uc.expected(g["filtered"], want["labels"], 4)


def _cluster(cuda, **kw):
    raw = _e2e()[0]
    return pipeline.cluster_points(_dev(raw, cuda), mc.E2E["eps"], mc.E2E["min_points"], mc.E2E["chunk_size"], **kw)


def _same_towers(a, b):
    assert len(a) == len(b)
    for s, t in zip(a, b):
        assert sorted(s) == sorted(t)
        for key in s:
            np.testing.assert_array_equal(np.asarray(s[key]), np.asarray(t[key]), err_msg=key)


def test_tower_table_upright(cuda):
    raw, g, labels, records = _e2e()
    cs = uc.table()
    before = pipeline.tower_table(_cluster(cuda, merge_threshold=6.0), extent_order=SORTED)
    towers = pipeline.tower_table(_cluster(cuda, merge_threshold=6.0), obb_mode="upright")
    assert [t["label"] for t in towers] == [0, 1, 2, 3] == [t["label"] for t in before]
    assert [len(t["points"]) for t in towers] == [1200, 1600, 1000, 1400]
    for t, rec in zip(towers, records):
        np.testing.assert_array_equal(t["points"].view(np.uint32), g["filtered"][labels == t["label"]].view(np.uint32))
        extents, transform = uc.tower_from_record(rec, cs)
        np.testing.assert_array_equal(t["center"], transform[:3, 3] + g["centroid"])
        np.testing.assert_array_equal(t["extent"], extents)
        np.testing.assert_array_equal(t["rotation"], transform[:3, :3])
        assert t["height"] == extents[2] == rec["zmax"] - rec["zmin"] and t["width"] == extents[0]
        assert t["aspect_ratio"] == extents[2] / extents[0]
        assert t["north_angle"] == pipeline.north_angle_deg(transform[:3, :3])
    # the new mode leaves no state behind: exact mode before and after it returns the same towers
    _same_towers(pipeline.tower_table(_cluster(cuda, merge_threshold=6.0), extent_order=SORTED), before)
    # without the merge the pieces of towers 1 and 3 are skipped by the centre de-dup, as in exact mode
    logs, exact_logs = [], []
    pieces = pipeline.tower_table(_cluster(cuda), obb_mode="upright", log=logs.append)
    exact = pipeline.tower_table(_cluster(cuda), extent_order=SORTED, log=exact_logs.append)
    assert [t["label"] for t in pieces] == [0, 1, 3, 4] == [t["label"] for t in exact]
    assert sum("跳过重复杆塔" in m for m in logs) == 2 == sum("跳过重复杆塔" in m for m in exact_logs)
    with pytest.raises(ValueError):
        pipeline.tower_table(_cluster(cuda), obb_mode="approximate")


def test_status_1_clusters_are_logged_as_failures(cuda):
    P, lab, K, want = _case("zero")
    x = _dev(P, cuda)
    perm, offsets, _ = ops.segment_by_label(_dev(lab, cuda), x, K)
    clusters = dict(ground=dict(points=x, centroid=np.zeros(3, dtype=np.float32)), nclusters=K, perm=perm, offsets=offsets)
    logs = []
    pipeline.tower_table(clusters, obb_mode="upright", log=logs.append)
    assert [m.split(" ")[1] for m in logs if "处理失败" in m] == ["簇10", "簇11", "簇12"]


# ------------------------------------------------------------------------------------------------------------- drop-in
def test_drop_in_knob(cuda, tmp_path, monkeypatch):
    from pointcloudhookup_amd import obb
    from pointcloudhookup_amd.utils import tower_extraction as te
    raw = _e2e()[0]
    scales, offsets = np.array([0.001, 0.001, 0.001]), np.array([437000.0, 3139000.0, 0.0])
    XYZ = np.round((raw.astype(np.float64) - offsets) / scales).astype(np.int32)
    path = str(tmp_path / "towers.las")
    las_bytes.build(path, XYZ, scales=scales, offsets=offsets)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(te, "CHUNK_SIZE", 2000)
    monkeypatch.setattr(te, "MERGE_THRESHOLD", 6.0)
    monkeypatch.setattr(te, "OBB_EXTENT_ORDER", SORTED)

    def run():
        for f in glob.glob(str(tmp_path / "output_towers" / "tower_*.las")):
            os.remove(f)
        logs, prog = [], []
        towers = te.extract_towers(path, progress_callback=prog.append, log_callback=logs.append, min_points=20)
        return towers, logs, prog, sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "output_towers" / "tower_*.las")))

    assert te.OBB_MODE == "exact"
    exact, exact_logs, exact_prog, exact_files = run()
    assert len(exact) == 4 and exact_files == [f"tower_{k}.las" for k in range(4)]
    # the upright run: no worker may be asked for, not even by the early start for large files
    started = []
    pool_before, size_before = obb._POOL, obb._POOL.size() if obb._POOL is not None else 0
    with monkeypatch.context() as m:
        m.setattr(te, "OBB_MODE", "upright")
        m.setattr(te, "PRESTART_BYTES", 0)
        m.setattr(obb, "prestart", lambda *a, **k: started.append("prestart"))
        m.setattr(obb, "pool", lambda *a, **k: started.append("pool"))
        towers, logs, prog, files = run()
    assert not started and obb._POOL is pool_before and (obb._POOL.size() if obb._POOL is not None else 0) == size_before
    assert len(towers) == 4 and files == exact_files and prog == exact_prog
    assert [len(t["points"]) for t in towers] == [len(t["points"]) for t in exact] == [1200, 1600, 1000, 1400]
    assert not any("处理失败" in m or "跳过重复杆塔" in m for m in logs)
    for t in towers:
        z = t["points"][:, 2].astype(np.float64)
        assert t["height"] == z.max() - z.min() and t["extent"][2] == t["height"] and t["rotation"][:, 2].tolist() == [0, 0, 1]
    # the knob back: logs and towers are those of the unmodified path
    again, again_logs, again_prog, again_files = run()
    assert again_logs == exact_logs and again_prog == exact_prog and again_files == exact_files
    _same_towers(again, exact)
