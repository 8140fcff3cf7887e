"""pch_plane_fit_f32 / pch_filter_plane_f32 through ops, the pipeline switch and the drop-in's module switch on the
GPU, bit for bit against the numpy statement of tests/plane_cases.py (uint64 views for doubles, uint32 for floats)."""
import functools
import re

import numpy as np
import pytest
import torch

import plane_cases as pc
from pointcloudhookup_amd import ops

pytestmark = pytest.mark.gpu

T = pc.COUNT_TILE
SIZES = [3, 63, 64, 65, T - 1, T, T + 1, 70_001, 300_007]
HYPS = [1, 63, 64, 65, 256]
FIT_CASES = [(n, H) for n in SIZES for H in HYPS] + [(70_001, 1000), (70_001, 4096)]
TABLE_N = 200_000


@functools.lru_cache(maxsize=None)
def _cloud(n):
    """(raw, truth, centroid, P) of the tilted corridor in the offset frame"""
    raw, truth = pc.tilted(n, 0.15, -0.05, offset=True, towers=3)
    centroid = np.mean(raw, axis=0)
    return raw, truth, centroid, pc.centre(raw, centroid)


@functools.lru_cache(maxsize=None)
def _fit(n, H):
    return pc.fit(_cloud(n)[3], pc.hypothesis_rows(n, H, 0))


@functools.lru_cache(maxsize=None)
def _table_ground():
    return pc.ground(_cloud(TABLE_N)[0], pc.hypothesis_rows(TABLE_N, 256, 0))


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same_fit(got, want):
    assert got["planes"].dtype == np.float64 and got["counts"].dtype == np.int64
    np.testing.assert_array_equal(got["planes"].view(np.uint64), want["planes"].view(np.uint64))
    np.testing.assert_array_equal(got["counts"], want["counts"])
    assert (got["best"], got["nvalid"], got["inliers"]) == (want["best"], want["nvalid"], want["inliers"])
    if want["plane"] is None:
        assert got["plane"] is None
    else:
        np.testing.assert_array_equal(got["plane"].view(np.uint64), want["plane"].view(np.uint64))


def _same_filter(got, want):
    pts, idx = got["points"].cpu().numpy(), got["index"].cpu().numpy()
    assert pts.dtype == np.float32 and idx.dtype == np.int32 and got["count"] == want["count"]
    np.testing.assert_array_equal(idx, want["index"])
    np.testing.assert_array_equal(pts.view(np.uint32), want["points"].view(np.uint32))
    np.testing.assert_array_equal(np.asarray(got["aabb"], dtype=np.float32).view(np.uint32),
                                  want["aabb"].view(np.uint32))


def test_count_tile_is_the_kernels():
    assert ops.PLANE_COUNT_TILE == T


@pytest.mark.parametrize("n,H", FIT_CASES)
def test_fit_equals_statement(cuda, n, H):
    raw, _, centroid, _ = _cloud(n)
    want = _fit(n, H)
    got = ops.plane_fit(_dev(raw, cuda), centroid, ops.plane_hypothesis_rows(n, H, 0))
    _same_fit(got, want)
    if n >= 63 and H >= 63:
        assert want["best"] >= 0 and 0 < want["nvalid"] < H       # both kinds of hypothesis are in the case


@pytest.mark.parametrize("n", [0, 1, 2])
def test_degenerate_sizes(cuda, n):
    """no row, or too few for a triple without a repeat: best = -1, the filter keeps nothing, the fused call raises"""
    raw = np.array([[1.0, 2.0, 3.0], [4.0, 6.0, 5.0]], dtype=np.float32)[:n]
    rows = np.zeros((7, 3), dtype=np.int64) if n == 0 else pc.hypothesis_rows(n, 7, 0)
    x = _dev(raw, cuda).reshape(-1, 3)
    got = ops.plane_fit(x, np.zeros(3, dtype=np.float32), rows)
    _same_fit(got, pc.fit(raw.reshape(-1, 3), rows))
    assert got["best"] == -1 and got["plane"] is None and got["nvalid"] == 0 and not got["counts"].any()
    for keep in ("above", "off_plane"):
        out = ops.filter_plane(x, np.zeros(3, dtype=np.float32), got, keep=keep)
        assert out["count"] == 0 and out["points"].shape == (0, 3) and not np.asarray(out["aabb"]).any()
    with pytest.raises(ValueError, match="no valid ground plane"):
        ops.ground_filter_plane(x)


def test_special_triples(cuda):
    raw, rows, valid = pc.special_cloud()
    zero = np.zeros(3, dtype=np.float32)
    want = pc.fit(pc.centre(raw, zero), rows)
    got = ops.plane_fit(_dev(raw, cuda), zero, rows)
    _same_fit(got, want)
    np.testing.assert_array_equal(got["planes"][:, 3] != 0, valid)
    assert not got["counts"][~valid].any() and (got["counts"][valid] >= 3).all()
    assert got["counts"][9] == got["counts"][11] == got["counts"].max() and got["best"] == 9    # tie: the lower index
    # the same table from the device, and a row outside the cloud where the host cannot check: invalid, not read
    far = rows.copy()
    far[1] = [0, 1, len(raw)]
    far[2] = [-1, 1, 2]
    got = ops.plane_fit(_dev(raw, cuda), zero, _dev(far, cuda))
    _same_fit(got, want)
    with pytest.raises(ValueError):
        ops.plane_fit(_dev(raw, cuda), zero, far)


@pytest.mark.parametrize("a,b", [(0.0, 0.0), (0.5, -0.25)])
def test_exact_boundaries(cuda, a, b):
    """rows exactly on |r| = 0.125 are inliers and dropped by off_plane, rows exactly at r = 3.0 are not kept by above,
    their float32 neighbours fall on the other side; NaN rows: never inliers, never above, kept by off_plane"""
    raw, rows, res = pc.boundary_cloud(a, b)
    zero = np.zeros(3, dtype=np.float32)
    x = _dev(raw, cuda)
    got = ops.plane_fit(x, zero, rows, residual_threshold=0.125)
    _same_fit(got, pc.fit(raw, rows, 0.125))
    with np.errstate(invalid="ignore"):
        inl, above = np.abs(res) <= 0.125, res > 3.0
    assert got["plane"].tolist() == [a, b, 0.0] and got["inliers"] == int(inl.sum())
    out = ops.filter_plane(x, zero, got, keep="above", offset=3.0)
    _same_filter(out, pc.filtered(raw, above))
    assert out["count"] == 10 and not np.isin(np.flatnonzero(res == 3.0), out["index"].cpu().numpy()).any()
    out = ops.filter_plane(x, zero, got, keep="off_plane", residual_threshold=0.125)
    _same_filter(out, pc.filtered(raw, ~inl))
    kept = out["index"].cpu().numpy()
    assert np.isin(np.flatnonzero(np.isnan(res)), kept).all() and not np.isin(np.flatnonzero(np.abs(res) == 0.125), kept).any()


@pytest.mark.parametrize("keep", ["above", "off_plane"])
@pytest.mark.parametrize("n", SIZES + [2047, 2048, 2049])
def test_filter_equals_statement(cuda, n, keep):
    raw, _, centroid, P = _cloud(n)
    f = _fit(n, 256)
    got = ops.filter_plane(_dev(raw, cuda), centroid, f["plane"], keep=keep)
    want = pc.filtered(P, pc.keep_mask(P, f["plane"], keep))
    _same_filter(got, want)
    if n >= 70_001:
        assert 0 < want["count"] < n
    nox = ops.filter_plane(_dev(raw, cuda), _dev(centroid, cuda), f, keep=keep, want_index=False)
    assert nox["index"] is None and nox["count"] == want["count"]
    np.testing.assert_array_equal(nox["points"].cpu().numpy().view(np.uint32), want["points"].view(np.uint32))


def test_filter_empty_and_all_kept(cuda):
    n = 70_001
    raw, _, centroid, P = _cloud(n)
    plane = _fit(n, 256)["plane"]
    x = _dev(raw, cuda)
    out = ops.filter_plane(x, centroid, plane, keep="above", offset=1e6)
    _same_filter(out, pc.filtered(P, np.zeros((n,), dtype=bool)))
    assert out["count"] == 0 and not np.asarray(out["aabb"]).any()
    out = ops.filter_plane(x, centroid, plane, keep="above", offset=-1e6)
    _same_filter(out, pc.filtered(P, np.ones((n,), dtype=bool)))
    assert out["count"] == n
    with pytest.raises(ValueError):
        ops.filter_plane(x, centroid, plane, keep="below")


@pytest.mark.parametrize("route", ["crop_aabb", "filter_plane", "filter_plane_tiles"])
def test_patchy_tiles(cuda, route):
    """empty tiles between live ones, a wave segment kept alone, a tile whose only kept row is its last (the facts are
    asserted on the mask in test_plane_host.py): every sweep on the shared compaction, bit for bit against numpy"""
    raw, mask = pc.patchy_cloud()
    zero, plane = np.zeros(3, dtype=np.float32), (0.0, 0.0, 0.0)
    want = pc.filtered(raw, mask)
    if route == "crop_aabb":
        x = _dev(raw.astype(np.float64), cuda)
        pts, idx = ops.crop_aabb(x, (-1e9, -1e9, 5.0), (1e9, 1e9, 15.0), want_index=True)
        assert idx.dtype == torch.int64
        np.testing.assert_array_equal(idx.cpu().numpy(), np.flatnonzero(mask))
        for got in (pts, ops.crop_aabb(x, (-1e9, -1e9, 5.0), (1e9, 1e9, 15.0))):
            np.testing.assert_array_equal(got.cpu().numpy().view(np.uint64), raw.astype(np.float64)[mask].view(np.uint64))
        return
    if route == "filter_plane":
        call = functools.partial(ops.filter_plane, _dev(raw, cuda), zero, plane, keep="above", offset=3.0)
    else:
        call = functools.partial(ops.filter_plane_tiles, _dev(raw, cuda), zero, dict(x0=0.0, y0=0.0, tile=200.0, nx=1, ny=1),
                                 dict(best=[0], planes=[plane]), keep="above", offset=3.0)
    _same_filter(call(), want)
    nox = call(want_index=False)
    assert nox["index"] is None and nox["count"] == want["count"]
    np.testing.assert_array_equal(nox["points"].cpu().numpy().view(np.uint32), want["points"].view(np.uint32))
    np.testing.assert_array_equal(np.asarray(nox["aabb"], dtype=np.float32).view(np.uint32), want["aabb"].view(np.uint32))


def _same_ground(got, want):
    _same_filter(got, want)
    np.testing.assert_array_equal(got["centroid"].view(np.uint32), want["centroid"].view(np.uint32))
    np.testing.assert_array_equal(got["plane"].view(np.uint64), want["plane"].view(np.uint64))
    assert got["base"].dtype == np.float32 and got["base"] == want["base"] and got["threshold"] == want["threshold"]
    for key in ("used_fallback", "count_at_offset", "count", "inliers", "nvalid", "best"):
        assert got[key] == want[key], key


def test_fallback(cuda):
    """fewer than min_keep rows above the offset: the rows above the fallback offset instead, both counts reported"""
    n = 70_001
    raw = _cloud(n)[0]
    rows = pc.hypothesis_rows(n, 64, 3)
    want = pc.ground(raw, rows, offset=40.0, fallback_offset=1.0, min_keep=1000)
    assert want["used_fallback"] and 0 < want["count_at_offset"] < 1000 <= want["count"]
    got = ops.ground_filter_plane(_dev(raw, cuda), rows=rows, offset=40.0, fallback_offset=1.0, min_keep=1000)
    _same_ground(got, want)
    assert got["threshold"] == np.float32(1.0)
    # off_plane mode has no fallback
    want = pc.ground(raw, rows, keep="off_plane", min_keep=10 ** 9)
    got = ops.ground_filter_plane(_dev(raw, cuda), rows=rows, keep="off_plane", min_keep=10 ** 9)
    _same_ground(got, want)
    assert not got["used_fallback"]


def test_fused_on_the_table_case(cuda):
    raw, truth, centroid, _ = _cloud(TABLE_N)
    want = _table_ground()
    got = ops.ground_filter_plane(_dev(raw, cuda))
    np.testing.assert_array_equal(got["centroid"].view(np.uint32), centroid.view(np.uint32))
    _same_ground(got, want)
    kept = np.zeros((TABLE_N,), dtype=bool)
    kept[got["index"].cpu().numpy()] = True
    assert int((kept != truth).sum()) <= 0.001 * int(truth.sum())
    nox = ops.ground_filter_plane(_dev(raw, cuda), want_index=False)
    assert nox["index"] is None and nox["count"] == want["count"]


def test_pipeline_switch(cuda):
    from pointcloudhookup_amd import pipeline
    raw = _cloud(TABLE_N)[0]
    want = _table_ground()
    x = _dev(raw, cuda)
    cl = pipeline.cluster_points(x, ground="plane", want_index=True)
    _same_ground(cl["ground"], want)
    labels, _, k = ops.dbscan(_dev(want["points"], cuda), 8.0, 80, pipeline.REF_CHUNK, aabb=want["aabb"])
    assert cl["nclusters"] == k and k >= 1
    lab = cl["labels"].cpu().numpy()
    np.testing.assert_array_equal(lab, labels.cpu().numpy())
    perm, offs = cl["perm"].cpu().numpy(), cl["offsets"].cpu().numpy()
    assert offs[0] == 0 and len(offs) == k + 1
    for c in range(k):
        np.testing.assert_array_equal(perm[offs[c]:offs[c + 1]], np.flatnonzero(lab == c))
    # keyword arguments reach the plane rule
    cl2 = pipeline.cluster_points(x, ground="plane", plane=dict(hypotheses=64, seed=2), segment=False)
    w2 = pc.ground(raw, pc.hypothesis_rows(TABLE_N, 64, 2))
    assert cl2["ground"]["best"] == w2["best"] and cl2["ground"]["count"] == w2["count"] and "perm" not in cl2
    # the default is the percentile rule, untouched
    a, b = pipeline.cluster_points(x), pipeline.cluster_points(x, ground="percentile")
    gf = ops.ground_filter(x, want_index=False)
    for cp in (a, b):
        assert "plane" not in cp["ground"] and cp["ground"]["count"] == gf["count"] > 2 * want["count"]
        assert torch.equal(cp["ground"]["points"], gf["points"]) and cp["nclusters"] == a["nclusters"]
        assert torch.equal(cp["labels"], a["labels"]) and torch.equal(cp["perm"], a["perm"])
    with pytest.raises(ValueError):
        pipeline.cluster_points(x, ground="tiles")


def test_drop_in_switch(cuda, tmp_path, monkeypatch):
    from oracle import voxel as ovx
    from pointcloudhookup_amd import las
    from pointcloudhookup_amd.utils import tower_extraction as te
    scales, offsets = np.array([0.001, 0.001, 0.001]), np.array([437000.0, 3139000.0, 0.0])
    raw = _cloud(TABLE_N)[0]
    XYZ = np.round((raw.astype(np.float64) - offsets) / scales).astype(np.int32)
    path = str(tmp_path / "slope.las")
    las.write(path, las.LasHeader(point_format=3, version=(1, 2), scales=scales, offsets=offsets), XYZ)
    back = np.stack([ovx.las_scaled(XYZ[:, a], scales[a], offsets[a]) for a in range(3)], axis=1).astype(np.float32)
    want = pc.ground(back, pc.hypothesis_rows(TABLE_N, 256, 0))
    monkeypatch.chdir(tmp_path)

    def kept(logs):
        hits = [m for m in logs if "保留点数" in m]
        assert len(hits) == 1
        return int(re.search(r"保留点数: (\d+)", hits[0]).group(1))

    assert te.GROUND_MODE == "percentile"
    logs = []
    assert isinstance(te.extract_towers(path, log_callback=logs.append), list)
    assert not any("地面平面" in m for m in logs)
    default_kept = kept(logs)
    monkeypatch.setattr(te, "GROUND_MODE", "plane")
    logs = []
    towers = te.extract_towers(path, log_callback=logs.append)
    assert isinstance(towers, list)
    a, b, c = want["plane"]
    line = f"📐 地面平面: z = {a:.6f}·x + {b:.6f}·y + {c:.3f}（内点 {want['inliers']}/{TABLE_N}）"
    assert line in logs and logs.index(line) == [i for i, m in enumerate(logs) if "保留点数" in m][0] + 1
    assert kept(logs) == want["count"] and default_kept > 2 * want["count"]
    # three rows on an 82 degree face: every triple repeats a row or fails the slope gate
    tiny = str(tmp_path / "tiny.las")
    las.write(tiny, las.LasHeader(point_format=3, version=(1, 2), scales=scales, offsets=offsets),
              np.array([[0, 0, 0], [1000, 0, 5000], [0, 1000, 5000]], dtype=np.int32))
    logs = []
    assert te.extract_towers(tiny, log_callback=logs.append) == []
    assert any(m.startswith("⚠️ 高度过滤失败") and "no valid ground plane" in m for m in logs)
