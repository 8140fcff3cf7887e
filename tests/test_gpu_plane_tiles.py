"""pch_plane_tiles_fit_f32 / pch_filter_plane_tiles_f32 through ops, the pipeline switch and the drop-in's module switch
on the GPU, bit for bit against the numpy statement of tests/plane_tiles_cases.py (uint64 views for doubles, uint32 for
floats)."""
import functools

import numpy as np
import pytest
import torch

import plane_cases as pc
import plane_tiles_cases as ptc
from pointcloudhookup_amd import _lib, ops

pytestmark = pytest.mark.gpu

ZERO = np.zeros(3, dtype=np.float32)
ALL = dict(x0=-1e7, y0=-1e7, tile=2e7, nx=1, ny=1)       # one tile that covers every finite cloud of these tests


def _dev(a, cuda):
    return torch.from_numpy(np.array(a)).to(cuda)           # a copy: the cached clouds are read-only


def _kept(index, n):
    kept = np.zeros((n,), dtype=bool)
    kept[index] = True
    return kept


def _same_tiles(got, want, tables=True):
    for key, dt in (("best", np.int32), ("inliers", np.int64), ("rows", np.int64), ("nvalid", np.int32)):
        assert got[key].dtype == dt, key
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    assert got["planes"].dtype == np.float64
    np.testing.assert_array_equal(got["planes"].view(np.uint64), want["planes"].view(np.uint64))
    if tables:
        np.testing.assert_array_equal(got["planes_table"].view(np.uint64), want["planes_table"].view(np.uint64))
        np.testing.assert_array_equal(got["counts_table"], want["counts_table"])


def _same_filter(got, want):
    pts, idx = got["points"].cpu().numpy(), got["index"].cpu().numpy()
    assert pts.dtype == np.float32 and idx.dtype == np.int32 and got["count"] == want["count"]
    np.testing.assert_array_equal(idx, want["index"])
    np.testing.assert_array_equal(pts.view(np.uint32), want["points"].view(np.uint32))
    np.testing.assert_array_equal(np.asarray(got["aabb"], dtype=np.float32).view(np.uint32),
                                  want["aabb"].view(np.uint32))


def _same_ground(got, want):
    _same_filter(got, want)
    np.testing.assert_array_equal(got["centroid"].view(np.uint32), want["centroid"].view(np.uint32))
    _same_tiles(got["tiles"], want["tiles"], tables=False)
    assert got["tiles"]["grid"] == want["tiles"]["grid"]
    if want["fallback_plane"] is None:
        assert got["fallback_plane"] is None and np.isnan(got["base"])
    else:
        np.testing.assert_array_equal(got["fallback_plane"].view(np.uint64), want["fallback_plane"].view(np.uint64))
        assert got["base"] == want["base"]
    assert got["base"].dtype == np.float32 and got["threshold"] == want["threshold"]
    for key in ("used_fallback", "count_at_offset", "count"):
        assert got[key] == want[key], key


@functools.lru_cache(maxsize=None)
def _tilted(n):
    raw, _ = pc.tilted(n, 0.15, -0.05, offset=True, towers=3)
    return raw, np.mean(raw, axis=0)


@functools.lru_cache(maxsize=None)
def _valley_want():
    return ptc.ground(ptc.valley()[0], **ptc.VALLEY_KW)


# ------------------------------------------------------------------ 1: a 1 x 1 grid is the global fit
@pytest.mark.parametrize("H", [1, 64, 65])
@pytest.mark.parametrize("n", [3, 64, 65, 1023, 1024, 1025, 70_001])
def test_one_tile_equals_global_fit(cuda, n, H):
    raw, centroid = _tilted(n)
    x = _dev(raw, cuda)
    table = ops.plane_tile_draws(H, 0)
    got = ops.plane_tiles_fit(x, centroid, ALL, table, min_tile_rows=1, want_tables=True)
    want = ops.plane_fit(x, centroid, table % n)
    np.testing.assert_array_equal(got["planes_table"][0].view(np.uint64), want["planes"].view(np.uint64))
    np.testing.assert_array_equal(got["counts_table"][0], want["counts"])
    assert (got["best"][0], got["nvalid"][0], got["inliers"][0]) == (want["best"], want["nvalid"], want["inliers"])
    assert got["rows"].tolist() == [n]
    if want["plane"] is not None:
        np.testing.assert_array_equal(got["planes"][0].view(np.uint64), want["plane"].view(np.uint64))
    if n >= 64 and H >= 64:
        assert want["best"] >= 0


# ------------------------------------------------------------------ 2: populations that straddle the pass size
@pytest.mark.parametrize("min_tile_rows", [1, 64])
def test_populations_straddle_the_pass(cuda, min_tile_rows):
    raw, grid = ptc.populations_cloud()
    assert ptc.PASS == ops.PLANE_COUNT_TILE == 1024
    P = pc.centre(raw, ZERO)
    table = ptc.draws(64, 0)
    want = ptc.fit(P, grid, table, min_tile_rows)
    np.testing.assert_array_equal(want["rows"], ptc.POPULATIONS)
    x = _dev(raw, cuda)
    got = ops.plane_tiles_fit(x, ZERO, grid, table, min_tile_rows=min_tile_rows, want_tables=True)
    _same_tiles(got, want)
    lean = ops.plane_tiles_fit(x, ZERO, grid, _dev(table, cuda), min_tile_rows=min_tile_rows)
    _same_tiles(lean, want, tables=False)
    assert "planes_table" not in lean and got["grid"] == grid
    has = np.array(ptc.POPULATIONS) >= max(min_tile_rows, 3)
    np.testing.assert_array_equal(got["best"] >= 0, has)
    fb = (0.1, 0.0, 1.2)
    for keep in ("above", "off_plane"):
        for fallback in (None, fb):
            out = ops.filter_plane_tiles(x, ZERO, grid, got, fallback=fallback, keep=keep)
            _same_filter(out, pc.filtered(P, ptc.keep_mask(P, grid, want, fallback, keep)))
            assert 0 < out["count"] < len(raw)
    nox = ops.filter_plane_tiles(x, ZERO, grid, want, fallback=fb, want_index=False)       # the statement's table
    assert nox["index"] is None and nox["count"] == int(ptc.keep_mask(P, grid, want, fb, "above").sum())


# ------------------------------------------------------------------ 3: the valley cloud
def test_valley(cuda):
    raw, truth = ptc.valley()
    want = _valley_want()
    x = _dev(raw, cuda)
    centroid, P, grid = want["centroid"], want["P"], want["tiles"]["grid"]
    assert ops.plane_tile_grid(x, centroid, 10.0) == grid and (grid["nx"], grid["ny"]) == (4, 11)
    assert ops.plane_tile_grid(x, _dev(centroid, cuda), 25.0) == ptc.grid_of(raw, centroid, 25.0)
    with pytest.raises(ValueError, match="smallest tile_size that fits"):
        ops.plane_tile_grid(x, centroid, 0.01)
    fit = ops.plane_tiles_fit(x, centroid, grid, ops.plane_tile_draws(64, 0), want_tables=True)
    _same_tiles(fit, want["tiles"])
    assert int((fit["best"] >= 0).sum()) == 30
    glob = ops.plane_fit(x, centroid, ops.plane_hypothesis_rows(len(raw), 256, 0))
    out = ops.filter_plane_tiles(x, centroid, grid, fit, fallback=glob)
    _same_filter(out, want)
    got = ops.ground_filter_plane_tiles(x, **ptc.VALLEY_KW)
    _same_ground(got, want)
    off = int((_kept(got["index"].cpu().numpy(), len(raw)) != truth).sum())
    assert (off, got["count"]) == (ptc.VALLEY_FIGURES[0], ptc.VALLEY_FIGURES[2]) and off <= 20
    # the defaults (20 m tiles, a 64-hypothesis fallback) and off_plane mode
    for kw in (dict(), dict(keep="off_plane", tile_size=25.0, seed=3)):
        _same_ground(ops.ground_filter_plane_tiles(x, **kw), ptc.ground(raw, **kw))


# ------------------------------------------------------------------ 4: rows without a tile
def test_rows_without_a_tile(cuda):
    raw = np.array(_tilted(70_001)[0][:20_000])
    centroid = np.mean(raw, axis=0)
    full = ptc.grid_of(raw, centroid, 8.0)
    grid = dict(full, x0=full["x0"] + 1.0, y0=full["y0"] + 20.0, nx=max(full["nx"] - 1, 1), ny=full["ny"] - 6)
    i1, i2 = np.flatnonzero(ptc.tile_of(pc.centre(raw, centroid), grid) >= 0)[[10, 500]]      # two rows inside the grid
    raw[5, 0], raw[77, 1], raw[19_999, 0], raw[i1, 2], raw[i2, 2] = np.nan, np.inf, -np.inf, np.nan, np.nan
    P = pc.centre(raw, centroid)
    table = ptc.draws(64, 1)
    want = ptc.fit(P, grid, table, 64)
    outside = want["tile"] < 0
    assert 1000 < outside.sum() < 19_000 and outside[[5, 77, 19_999]].all() and (want["best"] >= 0).any()
    x = _dev(raw, cuda)
    assert ops.plane_tile_grid(x, centroid, 8.0) == full       # the bounds skip the NaN and inf coordinates
    got = ops.plane_tiles_fit(x, centroid, grid, table, want_tables=True)
    _same_tiles(got, want)
    assert got["rows"].sum() == (~outside).sum()
    glob = pc.fit(P, pc.hypothesis_rows(len(raw), 64, 0))["plane"]
    for keep in ("above", "off_plane"):
        for fallback in (glob, None):
            out = ops.filter_plane_tiles(x, centroid, grid, got, fallback=fallback, keep=keep)
            mask = ptc.keep_mask(P, grid, want, fallback, keep)
            _same_filter(out, pc.filtered(P, mask))
            if fallback is None:
                assert not mask[outside].any()                  # no plane at all: dropped in either mode
    off = ptc.keep_mask(P, grid, want, glob, "off_plane")
    own = (want["tile"] >= 0) & (want["best"][np.maximum(want["tile"], 0)] >= 0)
    assert own[i1] and off[i1] and own[i2] and off[i2]          # NaN z in a tile with a plane: kept by off_plane
    assert off[5] and off[77]                                   # NaN x / inf y: on the fallback, NaN residual, kept
    assert not ptc.keep_mask(P, grid, want, glob, "above")[[5, i1, i2]].any()       # a NaN residual is never above


# ------------------------------------------------------------------ 5: the widest table, limits, empty cloud
def test_widest_table_and_limits(cuda):
    raw, centroid = _tilted(70_001)
    P = pc.centre(raw, centroid)
    g0 = ptc.grid_of(raw, centroid, 1.0)
    grid = dict(x0=g0["x0"] - 3.0, y0=g0["y0"] - 5.0, tile=0.5, nx=256, ny=256)
    table = ptc.draws(64, 0)
    want = ptc.fit(P, grid, table, 16)
    assert 0 < (want["rows"] > 0).sum() < 0.1 * 65536 and (want["best"] >= 0).sum() > 1000 and (want["tile"] >= 0).all()
    x = _dev(raw, cuda)
    got = ops.plane_tiles_fit(x, centroid, grid, table, min_tile_rows=16, want_tables=True)
    _same_tiles(got, want)
    out = ops.filter_plane_tiles(x, centroid, grid, got, fallback=None, keep="off_plane")
    _same_filter(out, pc.filtered(P, ptc.keep_mask(P, grid, want, None, "off_plane")))
    # beyond the limits
    with pytest.raises(ValueError):
        ops.plane_tiles_fit(x, centroid, dict(grid, nx=257), table)
    with pytest.raises(ValueError):
        ops.plane_tiles_fit(x, centroid, grid, ptc.draws(65, 0))
    with pytest.raises(ValueError):
        ops.filter_plane_tiles(x, centroid, dict(grid, ny=257), got)
    _c_abi_limits(x, centroid, cuda)
    # no row at all
    empty = ops.plane_tiles_fit(x[:0], centroid, ptc.populations_cloud()[1], table, want_tables=True)
    assert (empty["best"] == -1).all() and not empty["rows"].any() and not empty["counts_table"].any()
    assert not empty["planes_table"].any() and len(empty["best"]) == 9
    out = ops.filter_plane_tiles(x[:0], centroid, ptc.populations_cloud()[1], empty, fallback=(0.0, 0.0, 0.0))
    assert out["count"] == 0 and out["points"].shape == (0, 3)
    with pytest.raises(ValueError, match="no valid ground plane"):
        ops.ground_filter_plane_tiles(x[:0])


def _c_abi_limits(x, centroid, cuda):
    """PCH_ERR_ARG for 65 537 tiles, for tiles x hypotheses beyond 2^22 and for a bad tile edge; PCH_ERR_WORKSPACE for a
    workspace one byte short - none of them launches anything; the exact size is enough"""
    import ctypes as C
    L = _lib.lib()
    n, H = x.shape[0], 64
    cen = _dev(np.asarray(centroid, dtype=np.float32), cuda)
    table = _dev(ptc.draws(65, 0), cuda)
    best = torch.zeros((65536 * 40,), dtype=torch.uint8, device=cuda)
    ws = torch.empty((L.pch_plane_tiles_fit_ws_bytes(n, 65536, H) + 256,), dtype=torch.uint8, device=cuda)
    stream = torch.cuda.current_stream().cuda_stream

    def fit(grid, H, ws_bytes):
        g = _lib.PlaneGridC(grid["x0"], grid["y0"], grid["tile"], grid["nx"], grid["ny"])
        return L.pch_plane_tiles_fit_f32(x.data_ptr(), n, cen.data_ptr(), C.cast(C.pointer(g), C.c_void_p),
                                         table.data_ptr(), H, 64, 0.1, 0.5, best.data_ptr(), 0, 0, 0, ws.data_ptr(),
                                         ws_bytes, stream)

    base = dict(x0=0.0, y0=0.0, tile=1.0, nx=256, ny=256)
    arg, short = -1, -2
    assert _lib.ERR_NAMES[arg] == "PCH_ERR_ARG" and _lib.ERR_NAMES[short] == "PCH_ERR_WORKSPACE"
    assert fit(dict(base, nx=257), H, ws.numel()) == arg and fit(dict(base, nx=65537, ny=1), H, ws.numel()) == arg
    assert fit(base, 65, ws.numel()) == arg
    for tile in (0.0, -1.0, float("inf"), float("nan")):
        assert fit(dict(base, tile=tile), H, ws.numel()) == arg
    assert fit(dict(base, nx=0), H, ws.numel()) == arg
    need = L.pch_plane_tiles_fit_ws_bytes(n, 65536, H)
    assert fit(base, H, need - 1) == short and fit(base, H, need) == 0
    g = _lib.PlaneGridC(0.0, 0.0, 1.0, 4, 4)
    cnt = torch.zeros((1,), dtype=torch.int64, device=cuda)
    pts = torch.empty((n, 3), dtype=torch.float32, device=cuda)
    need = L.pch_filter_plane_tiles_ws_bytes(n, 16)
    rc = L.pch_filter_plane_tiles_f32(x.data_ptr(), n, cen.data_ptr(), C.cast(C.pointer(g), C.c_void_p), best.data_ptr(),
                                      0, 0, 3.0, pts.data_ptr(), 0, cnt.data_ptr(), 0, ws.data_ptr(), need - 1, stream)
    assert rc == short
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 6: ties and gates
def test_ties_and_gates(cuda):
    """the same draw twice: the smaller h wins; a tile of rows on a steep face has no plane and falls back"""
    rng = np.random.Generator(np.random.PCG64(11))
    m = 700
    flat = np.stack([rng.uniform(0.5, 7.5, m), rng.uniform(0.5, 7.5, m), rng.normal(0.0, 0.02, m)], axis=1)
    xs = rng.uniform(8.5, 15.5, m)
    steep = np.stack([xs, rng.uniform(0.5, 7.5, m), 6.0 * (xs - 8.0) + rng.normal(0.0, 0.001, m)], axis=1)   # 80 degrees
    raw = np.concatenate([flat, steep])[rng.permutation(2 * m)].astype(np.float32)
    grid = dict(x0=0.0, y0=0.0, tile=8.0, nx=2, ny=1)
    table = ptc.draws(64, 2)
    table[40] = table[7]
    table[3] = table[7]
    P = pc.centre(raw, ZERO)
    want = ptc.fit(P, grid, table, 64)
    c = want["counts_table"][0]
    assert c[3] == c[7] == c[40] and want["planes_table"][0, 3, 3] == 1.0
    assert want["nvalid"][1] == 0 and want["best"][1] == -1 and want["best"][0] >= 0
    x = _dev(raw, cuda)
    got = ops.plane_tiles_fit(x, ZERO, grid, table, want_tables=True)
    _same_tiles(got, want)
    # make the tied triple the winner: only the three copies are left valid candidates of the maximum
    only = np.repeat(table[7:8], 5, axis=0)
    w2 = ptc.fit(P, grid, only, 64)
    g2 = ops.plane_tiles_fit(x, ZERO, grid, only, want_tables=True)
    _same_tiles(g2, w2)
    assert g2["best"][0] == 0 and g2["nvalid"][0] == 5 and g2["best"][1] == -1
    fb = (6.0, 0.0, -48.0)                                      # the steep face itself, as the fallback
    out = ops.filter_plane_tiles(x, ZERO, grid, got, fallback=fb, keep="off_plane", residual_threshold=0.1)
    mask = ptc.keep_mask(P, grid, want, fb, "off_plane", thr=0.1)
    _same_filter(out, pc.filtered(P, mask))
    assert mask[want["tile"] == 1].sum() < 0.05 * m             # the face's rows went to the fallback and lie on it
    none = ops.filter_plane_tiles(x, ZERO, grid, got, fallback=None, keep="off_plane")
    assert not np.isin(np.flatnonzero(want["tile"] == 1), none["index"].cpu().numpy()).any()


# ------------------------------------------------------------------ 7: the fallback offset
def test_fallback_offset_and_no_index(cuda):
    raw = ptc.valley()[0]
    x = _dev(raw, cuda)
    kw = dict(ptc.VALLEY_KW, offset=40.0, fallback_offset=1.0, min_keep=1000)
    want = ptc.ground(raw, **kw)
    assert want["used_fallback"] and 0 < want["count_at_offset"] < 1000 <= want["count"]
    got = ops.ground_filter_plane_tiles(x, **kw)
    _same_ground(got, want)
    assert got["threshold"] == np.float32(1.0)
    nox = ops.ground_filter_plane_tiles(x, want_index=False, **kw)
    assert nox["index"] is None and nox["count"] == want["count"] and nox["used_fallback"]
    np.testing.assert_array_equal(nox["points"].cpu().numpy().view(np.uint32), want["points"].view(np.uint32))
    off = ops.ground_filter_plane_tiles(x, **dict(kw, keep="off_plane", min_keep=10 ** 9))
    assert not off["used_fallback"]                             # off_plane mode has no fallback offset


# ------------------------------------------------------------------ 8: the pipeline switch
def test_pipeline_switch(cuda):
    from pointcloudhookup_amd import pipeline
    raw = ptc.valley()[0]
    want = _valley_want()
    x = _dev(raw, cuda)
    cl = pipeline.cluster_points(x, ground="plane_tiles", plane=dict(ptc.VALLEY_KW), want_index=True)
    _same_ground(cl["ground"], want)
    labels, _, k = ops.dbscan(_dev(want["points"], cuda), 8.0, 80, pipeline.REF_CHUNK, aabb=want["aabb"])
    assert cl["nclusters"] == k and k >= 1
    lab = cl["labels"].cpu().numpy()
    np.testing.assert_array_equal(lab, labels.cpu().numpy())
    perm, offs = cl["perm"].cpu().numpy(), cl["offsets"].cpu().numpy()
    assert offs[0] == 0 and len(offs) == k + 1
    for c in range(k):
        np.testing.assert_array_equal(perm[offs[c]:offs[c + 1]], np.flatnonzero(lab == c))
    # keyword arguments reach the rule
    kw = dict(tile_size=25.0, hypotheses=32, seed=2, fallback_hypotheses=16)
    cl2 = pipeline.cluster_points(x, ground="plane_tiles", plane=kw, segment=False)
    w2 = ptc.ground(raw, **kw)
    assert cl2["ground"]["count"] == w2["count"] and "perm" not in cl2 and cl2["ground"]["index"] is None
    np.testing.assert_array_equal(cl2["ground"]["tiles"]["best"], w2["tiles"]["best"])
    # the other rules are untouched
    a, b = pipeline.cluster_points(x), pipeline.cluster_points(x, ground="percentile")
    gf = ops.ground_filter(x, want_index=False)
    for cp in (a, b):
        assert "tiles" not in cp["ground"] and cp["ground"]["count"] == gf["count"] > 2 * want["count"]
        assert torch.equal(cp["ground"]["points"], gf["points"]) and cp["nclusters"] == a["nclusters"]
        assert torch.equal(cp["labels"], a["labels"]) and torch.equal(cp["perm"], a["perm"])
    one = pipeline.cluster_points(x, ground="plane", want_index=True, segment=False)
    w1 = pc.ground(raw, pc.hypothesis_rows(len(raw), 256, 0))
    assert "tiles" not in one["ground"] and one["ground"]["count"] == w1["count"]
    np.testing.assert_array_equal(one["ground"]["index"].cpu().numpy(), w1["index"])
    with pytest.raises(ValueError):
        pipeline.cluster_points(x, ground="tiles")


# ------------------------------------------------------------------ 9: the drop-in's module switch
def test_drop_in_switch(cuda, tmp_path, monkeypatch):
    from oracle import voxel as ovx
    from pointcloudhookup_amd import las
    from pointcloudhookup_amd.utils import tower_extraction as te
    scales, offsets = np.array([0.001, 0.001, 0.001]), np.array([437000.0, 3139000.0, 0.0])
    raw = ptc.valley()[0]
    XYZ = np.round((raw.astype(np.float64) - offsets) / scales).astype(np.int32)
    path = str(tmp_path / "valley.las")
    las.write(path, las.LasHeader(point_format=3, version=(1, 2), scales=scales, offsets=offsets), XYZ)
    back = np.stack([ovx.las_scaled(XYZ[:, a], scales[a], offsets[a]) for a in range(3)], axis=1).astype(np.float32)
    monkeypatch.chdir(tmp_path)
    assert te.GROUND_MODE == "percentile" and te.GROUND_TILE == 20.0
    logs = []
    assert isinstance(te.extract_towers(path, log_callback=logs.append), list)
    assert not any("分块地面平面" in m or "地面平面" in m for m in logs)
    monkeypatch.setattr(te, "GROUND_MODE", "plane_tiles")
    for tile in (20.0, 10.0):
        monkeypatch.setattr(te, "GROUND_TILE", tile)
        want = ptc.ground(back, tile_size=tile)
        logs = []
        assert isinstance(te.extract_towers(path, log_callback=logs.append), list)
        own, occupied = int((want["tiles"]["best"] >= 0).sum()), int((want["tiles"]["rows"] > 0).sum())
        a, b, c = want["fallback_plane"]
        line = (f"📐 分块地面平面: 分块 {tile:g} m，独立平面 {own}/{occupied} 块，"
                f"回退平面: z = {a:.6f}·x + {b:.6f}·y + {c:.3f}")
        kept = [i for i, m in enumerate(logs) if "保留点数" in m]
        assert len(kept) == 1 and logs[kept[0]] == f"✅ 高度过滤完成，保留点数: {want['count']}"
        assert line in logs and logs.index(line) == kept[0] + 1 and 0 < own <= occupied
        assert not any(m.startswith("📐 地面平面") for m in logs)
