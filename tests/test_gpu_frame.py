"""The LAS-integer frame of stage B on the device (pch_ground_filter_las_i32, called through ctypes) against the
numpy statement of tests/frame_cases.py, bit for bit; the argument errors; and the drop-in end to end."""
import ctypes

import numpy as np
import pytest
import torch

import frame_cases as fc
import las_bytes
from oracle import dbscan as odb
from oracle import towers as otw
from pointcloudhookup_amd import _lib, ops

pytestmark = pytest.mark.gpu

T = ops.FRAME_TILE
ORDER = "trimesh_sorted"          # the extent convention under which all three towers of the corridor are accepted


def run_library(dev, XYZ, scales, pct, offset, fallback_offset, min_keep, want_index=True, misalign=False):
    """one call of the entry point on its own buffers; returns the record and the kept rows as numpy"""
    L = _lib.lib()
    n = len(XYZ)
    flat = torch.from_numpy(np.ascontiguousarray(XYZ, dtype=np.int32).reshape(-1))
    if misalign:                                                    # the rows start 4 bytes behind a 16-byte boundary
        buf = torch.empty(3 * n + 1, dtype=torch.int32, device=dev)
        buf[1:] = flat.to(dev)
        X = buf[1:]
        assert X.data_ptr() % 16 == 4
    else:
        X = flat.to(dev)
        assert X.data_ptr() % 16 == 0
    out_points = torch.full((n, 3), float("nan"), dtype=torch.float32, device=dev)
    out_index = torch.full((n,), -7, dtype=torch.int32, device=dev) if want_index else None
    rec = torch.zeros(ctypes.sizeof(_lib.LasFrameC), dtype=torch.uint8, device=dev)
    nb = L.pch_ground_filter_las_ws_bytes(n)
    ws = torch.full((nb,), 0xA5, dtype=torch.uint8, device=dev)      # the call must clear what it relies on
    sc = (ctypes.c_double * 3)(*[float(v) for v in scales])
    rc = L.pch_ground_filter_las_i32(X.data_ptr(), n, ctypes.cast(sc, ctypes.c_void_p), float(pct), float(offset),
                                     float(fallback_offset), int(min_keep), out_points.data_ptr(),
                                     out_index.data_ptr() if want_index else None, rec.data_ptr(), ws.data_ptr(), nb,
                                     torch.cuda.current_stream().cuda_stream)
    assert rc == 0, L.pch_last_error()
    f = _lib.LasFrameC.from_buffer_copy(rec.cpu().numpy().tobytes())
    m = int(f.count)
    assert 0 <= m <= n
    return f, out_points[:m].cpu().numpy(), (out_index[:m].cpu().numpy() if want_index else None), out_points


def assert_equals_statement(f, points, index, st):
    assert list(f.centroid) == st["C"].tolist()
    assert f.count == st["count"] and f.count_at_offset == st["count_at_offset"]
    assert bool(f.used_fallback) == st["used_fallback"]
    assert np.float32(f.base).view(np.uint32) == st["base"].view(np.uint32), (f.base, st["base"])
    assert np.float32(f.threshold).view(np.uint32) == st["threshold"].view(np.uint32)
    assert np.array_equal(points.view(np.uint32), st["points"].view(np.uint32))
    if index is not None:
        assert np.array_equal(index, st["index"])
    assert np.array_equal(np.array(list(f.aabb), dtype=np.float32).view(np.uint32), st["aabb"].view(np.uint32))


@pytest.mark.parametrize("case", fc.all_cases(T), ids=lambda c: c["name"])
def test_library_equals_the_statement(cuda, case):
    args = [case[k] for k in ("XYZ", "scales", "pct", "offset", "fallback_offset", "min_keep")]
    f, points, index, full = run_library(cuda, *args)
    st = fc.statement(*args)
    assert_equals_statement(f, points, index, st)
    # nothing is written behind the kept rows (of either threshold: the fallback's sweep writes over the first one's)
    assert bool(torch.isnan(full[max(f.count, f.count_at_offset):]).all())


@pytest.mark.parametrize("n", [5, 1025, 3 * T + 5])
def test_rows_off_a_16_byte_boundary_and_no_index(cuda, n):
    """the element-by-element loaders of the sweeps, and out_index = NULL"""
    X = fc.corridor_records(n, 77)
    f, points, index, _ = run_library(cuda, X, (0.001,) * 3, 25.0, 3.0, 1.0, 10, want_index=False, misalign=True)
    assert index is None
    assert_equals_statement(f, points, None, fc.statement(X, (0.001,) * 3, 25.0, 3.0, 1.0, 10))


def test_ops_wrapper_and_pipeline(cuda):
    from pointcloudhookup_amd import pipeline
    X, s, o = fc.tower_corridor(60_000)
    st = fc.statement(X, s)
    dev = torch.from_numpy(X).to(cuda)
    gf = ops.ground_filter_las(dev, s, o, want_index=True)
    assert gf["frame"] == "las" and gf["centroid"].dtype == np.float64 and gf["centroid_int"].dtype == np.int64
    assert np.array_equal(gf["centroid_int"], st["C"])
    assert np.array_equal(gf["centroid"], fc.centroid_world(st["C"], s, o))
    assert gf["count"] == st["count"] and gf["used_fallback"] == st["used_fallback"]
    assert np.array_equal(gf["points"].cpu().numpy().view(np.uint32), st["points"].view(np.uint32))
    assert np.array_equal(gf["index"].cpu().numpy(), st["index"]) and np.array_equal(gf["aabb"], st["aabb"])
    cl = pipeline.cluster_points_las(dev, s, o, 8.0, 80, 50000, merge_threshold=6.0)
    plain = pipeline.cluster_points_las(dev, s, o, 8.0, 80, 50000)
    assert torch.equal(plain["ground"]["points"], gf["points"]) and plain["ground"]["index"] is None
    assert {"labels", "nclusters", "perm", "offsets", "stats", "ground"} <= set(plain)
    assert "merge" in cl and cl["nclusters"] <= plain["nclusters"] and plain["nclusters"] >= 3


def test_argument_errors(cuda):
    L = _lib.lib()
    n = 100
    X = torch.from_numpy(fc.corridor_records(n, 5)).to(cuda)
    pts = torch.empty((n, 3), dtype=torch.float32, device=cuda)
    rec = torch.zeros(ctypes.sizeof(_lib.LasFrameC), dtype=torch.uint8, device=cuda)
    nb = L.pch_ground_filter_las_ws_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream

    def call(n=n, scales=(0.001, 0.001, 0.001), pct=25.0, ws_bytes=nb):
        sc = (ctypes.c_double * 3)(*scales)
        return L.pch_ground_filter_las_i32(X.data_ptr(), n, ctypes.cast(sc, ctypes.c_void_p), pct, 3.0, 1.0, 10,
                                           pts.data_ptr(), None, rec.data_ptr(), ws.data_ptr(), ws_bytes, st)

    assert call() == 0
    for bad in (dict(n=0), dict(n=-1), dict(n=2 ** 31), dict(n=2 ** 40),
                dict(scales=(0.0, 0.001, 0.001)), dict(scales=(0.001, -0.001, 0.001)),
                dict(scales=(0.001, 0.001, float("nan"))), dict(scales=(float("inf"), 0.001, 0.001)),
                dict(pct=-0.001), dict(pct=100.001), dict(pct=float("nan"))):
        assert call(**bad) == -1, bad                               # PCH_ERR_ARG
        assert L.pch_last_error()
    assert call(ws_bytes=nb - 1) == -2 and call(ws_bytes=0) == -2   # PCH_ERR_WORKSPACE
    assert b"workspace too small" in L.pch_last_error()
    torch.cuda.synchronize()
    assert call() == 0


# ------------------------------------------------------------------ end to end through the drop-in
@pytest.fixture(scope="module")
def corridor_file(tmp_path_factory):
    """the quantised 200 000-row three-tower corridor as a byte-built LAS file, and the statement on its records"""
    d = tmp_path_factory.mktemp("frame")
    X, s, o = fc.tower_corridor(200_000)
    path = str(d / "corridor.las")
    las_bytes.build(path, X, point_format=3, version=(1, 2), scales=s, offsets=o)
    return path, X, s, o, fc.statement(X, s, 25.0, 3.0, 1.0, 1000), d


def _expected_towers(st, s, o, oracle_points=None):
    pts = st["points"] if oracle_points is None else oracle_points
    labels = odb.dbscan_chunked(pts, 8.0, 80, 50000, fit="c")
    cw = fc.centroid_world(st["C"], s, o)
    towers, ncand = otw.towers_from_labels(pts, labels, cw, extent_order=ORDER)
    return labels, towers, ncand, cw


def _assert_towers(got, want):
    assert len(got) == len(want)
    for t, r in zip(got, want):
        assert set(t) == {"center", "rotation", "extent", "height", "width", "north_angle", "points"}
        for k in ("center", "extent", "rotation", "north_angle", "height", "width"):
            assert np.array_equal(np.asarray(t[k]), np.asarray(r[k])), k
        assert np.array_equal(t["points"].view(np.uint32), r["points"].view(np.uint32))


def _rows_multiset(a):
    rows, counts = np.unique(a, axis=0, return_counts=True)
    return {tuple(r): int(c) for r, c in zip(rows.tolist(), counts.tolist())}


def test_extract_towers_in_the_las_frame(cuda, oracle_clib, corridor_file, monkeypatch):
    from pointcloudhookup_amd.utils import tower_extraction as te
    path, X, s, o, st, d = corridor_file
    labels, want, ncand, cw = _expected_towers(st, s, o)
    assert len(want) == 3
    # labels and cluster count of the device run on the statement's rows
    dev_labels, _, k = ops.dbscan(torch.from_numpy(st["points"]).to(cuda), 8.0, 80, 50000, aabb=st["aabb"])
    assert k == ncand and np.array_equal(dev_labels.cpu().numpy(), labels)
    work = d / "las_frame"
    work.mkdir()
    monkeypatch.chdir(work)
    monkeypatch.setattr(te, "FRAME", "las")
    monkeypatch.setattr(te, "OBB_EXTENT_ORDER", ORDER)
    logs, prog = [], []
    got = te.extract_towers(path, progress_callback=prog.append, log_callback=logs.append)
    _assert_towers(got, want)
    assert f"✅ 点云读取完成，总点数: {len(X)}" in logs and f"✅ 高度过滤完成，保留点数: {st['count']}" in logs
    assert f"\n=== 开始杆塔检测（候选簇：{ncand}个） ===" in logs and logs[-1] == "✅ 杆塔提取完成"
    extra = [m for m in logs if m.startswith("📐 LAS整数坐标系")]
    assert len(extra) == 1 and str(int(st["C"][1])) in extra[0] and f"{cw[1]:.3f}" in extra[0]
    assert logs.index(extra[0]) == logs.index(f"✅ 高度过滤完成，保留点数: {st['count']}") + 1
    assert prog[:3] == [5, 10, 20] and prog[-1] == 100 and prog == sorted(prog)
    # every record of a per-tower file is one of the input's records, as often as there at most
    have = _rows_multiset(X)
    for r in want:
        rec = las_bytes.parse_xyz(str(work / "output_towers" / f"tower_{r['label']}.las"))
        assert rec["n"] == len(r["points"])
        assert np.array_equal(rec["XYZ"], X[st["index"]][labels == r["label"]])
        for row, c in _rows_multiset(rec["XYZ"]).items():
            assert have.get(row, 0) >= c, row


def test_frame_unset_gives_the_reference_frames_towers(cuda, oracle_clib, corridor_file, monkeypatch):
    """FRAME unset: the towers are those of the reference's float32 frame (the oracle's), as before"""
    from oracle import voxel as ovx
    from pointcloudhookup_amd.utils import tower_extraction as te
    path, X, s, o, st, d = corridor_file
    work = d / "reference_frame"
    work.mkdir()
    monkeypatch.chdir(work)
    assert te.FRAME == "reference"
    monkeypatch.setattr(te, "OBB_EXTENT_ORDER", ORDER)
    logs = []
    got = te.extract_towers(path, log_callback=logs.append)
    xyz = np.stack([ovx.las_scaled(X[:, a], s[a], o[a]) for a in range(3)], axis=1)
    ref = otw.extract_towers_arrays(xyz[:, 0], xyz[:, 1], xyz[:, 2], fit="c", extent_order=ORDER)
    _assert_towers(got, ref["towers"])
    assert not [m for m in logs if m.startswith("📐 LAS整数坐标系")]


def test_resident_hand_off_in_the_las_frame(cuda, oracle_clib, corridor_file, monkeypatch):
    """run_voxel_downsampling leaves its records on the device; extract_towers with FRAME = "las" takes them without a
    file read, without las_scale and without cast_f32, and gives the towers of the statement on those records"""
    from pointcloudhookup_amd import las as _las
    from pointcloudhookup_amd.ui import import_PC
    from pointcloudhookup_amd.utils import tower_extraction as te
    path, X, s, o, st, d = corridor_file
    work = d / "resident"
    work.mkdir()
    monkeypatch.chdir(work)
    monkeypatch.setenv("PCH_RESIDENT_HANDOFF", "1")
    out = str(work / "output" / "point_2.las")
    import_PC.run_voxel_downsampling(path, out, 0.1, 500000)
    monkeypatch.setattr(te, "FRAME", "las")
    monkeypatch.setattr(te, "OBB_EXTENT_ORDER", ORDER)
    monkeypatch.setattr(_las, "read_device", lambda *a: pytest.fail("the file was read although its records were resident"))
    monkeypatch.setattr(ops, "las_scale", lambda *a: pytest.fail("las_scale in the LAS frame"))
    monkeypatch.setattr(ops, "cast_f32", lambda *a: pytest.fail("cast_f32 in the LAS frame"))
    got = te.extract_towers(out, log_callback=lambda m: None)
    monkeypatch.undo()
    V = las_bytes.parse_xyz(out)["XYZ"]
    stv = fc.statement(V, s, 25.0, 3.0, 1.0, 1000)
    labels, want, ncand, cw = _expected_towers(stv, s, o)
    assert len(want) == 3
    _assert_towers(got, want)
    have = _rows_multiset(V)
    for r in want:
        rec = las_bytes.parse_xyz(str(work / "output_towers" / f"tower_{r['label']}.las"))
        for row, c in _rows_multiset(rec["XYZ"]).items():
            assert have.get(row, 0) >= c, row
