"""The LAS-integer frame of stage B without a device: the numpy statement (tests/frame_cases.py) against an
independent formulation, what the frame buys at projected-CRS magnitudes, the C ABI, and the knobs."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import frame_cases as fc
from pointcloudhookup_amd import _lib, ops, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pch_ground_filter_las_ws_bytes", "pch_ground_filter_las_i32")


# ------------------------------------------------------------------ (a) the statement
@pytest.mark.parametrize("case", fc.all_cases(ops.FRAME_TILE), ids=lambda c: c["name"])
def test_statement_agrees_with_an_independent_formulation(case):
    """centroid by // on Python integers, threshold by a live np.percentile, kept rows by a boolean mask"""
    X, s = case["XYZ"], case["scales"]
    n = len(X)
    st = fc.statement(X, s, case["pct"], case["offset"], case["fallback_offset"], case["min_keep"])
    C = [int(X[:, j].astype(np.int64).sum()) // n for j in range(3)]
    assert st["C"].tolist() == C
    p = np.empty((n, 3), dtype=np.float32)
    for j in range(3):
        p[:, j] = (X[:, j].astype(np.int64) - C[j]).astype(np.float64) * s[j]
    assert np.array_equal(st["p"].view(np.uint32), p.view(np.uint32))
    base = np.percentile(p[:, 2], case["pct"])
    assert base.dtype == np.float32 and base.view(np.uint32) == st["base"].view(np.uint32)
    mask = p[:, 2] > base + np.float32(case["offset"])
    assert st["count_at_offset"] == int(mask.sum())
    assert st["used_fallback"] == (int(mask.sum()) < case["min_keep"])
    if st["used_fallback"]:
        mask = p[:, 2] > base + np.float32(case["fallback_offset"])
    assert st["count"] == int(mask.sum())
    assert np.array_equal(st["points"].view(np.uint32), p[mask].view(np.uint32))
    assert np.array_equal(st["index"], np.nonzero(mask)[0])
    if st["count"]:
        assert np.array_equal(st["aabb"], np.concatenate([p[mask].min(0), p[mask].max(0)]))
    else:
        assert not st["aabb"].any()


def test_floor_division_is_not_truncation():
    for S, n in ((-3, 2), (-4, 3), (-1, 100), (-100, 100), (3, 2), (0, 5), (-(2 ** 61) - 1, 2 ** 31 - 1)):
        assert fc.floor_div(S, n) == S // n
    assert fc.centroid_int(np.array([[-1, 0, 0], [-2, 0, 0]], dtype=np.int32))[0] == -2       # trunc would say -1


def test_cases_cover_what_they_claim():
    T = ops.FRAME_TILE
    assert {1, 2, 3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 5, 65 * T + 7} <= set(fc.sizes(T))
    cases = {c["name"]: c for c in fc.all_cases(T)}
    st = lambda name: fc.statement(*(cases[name][k] for k in ("XYZ", "scales", "pct", "offset", "fallback_offset",
                                                             "min_keep")))
    big = cases["columns all INT32_MAX / all INT32_MIN"]["XYZ"]
    assert abs(int(big[:, 0].astype(np.int64).sum())) > 2 ** 47 and len(big) == 100_000
    r = st("columns all INT32_MAX / all INT32_MIN")
    assert not r["p"][:, :2].any() and r["C"][0] == fc.I32_MAX and r["C"][1] == fc.I32_MIN
    r = st("alternating INT32_MIN / INT32_MAX, n=100000")
    assert r["C"][0] == -1 and r["C"][1] == -1            # sum -n/2: floor(-0.5) = -1, trunc would give 0
    assert r["p"][:, 0].max() == np.float32(2 ** 31 * 0.001)
    r = st("all Z equal: nothing kept, fallback included")
    assert r["count"] == 0 and r["used_fallback"] and not r["aabb"].any()
    r = st("fallback engages")
    assert r["used_fallback"] and r["count_at_offset"] < 1000 <= r["count"]
    r = st("min_keep = 0")
    assert not r["used_fallback"] and r["count"] == r["count_at_offset"] == 0
    gammas = {float(fc.pct_index(n, q)[2]) for n in (2, 3, 4, 5) for q in (25.0, 50.0, 99.9)}
    assert any(0 < g < 0.5 for g in gammas) and any(g >= 0.5 for g in gammas)


# ------------------------------------------------------------------ (b) what the frame buys
def test_rows_map_back_to_their_own_las_integers():
    """300 001 rows of a 10 km corridor at EPSG:4547 magnitudes, LAS scale 0.001.  world = X * s + o in float64.
    In the frame, p + centroid_world - world = p - (X - C) * s as real numbers (the world-sized terms cancel), and p is
    the float32 nearest to float64((X - C) * s): the difference is at most half a float32 ulp of |p| per element.  It
    is taken in that cancelled form, where every operation below is exact in float64; the literal float64 expression
    adds its own roundings at world magnitude (three of at most half a float64 ulp of 3.2e6 each), which it is given.
    Half an ulp stays under half the scale (0.0005 m) while |p| < 16 384 m, where the float32 ulp is 2^-10 m at most:
    so every row rounds back to its own record."""
    X, s, o = fc.epsg_corridor()
    assert len(X) == 300_001
    world = X.astype(np.float64) * s + o
    C = fc.centroid_int(X)
    cw = fc.centroid_world(C, s, o)
    p = fc.centre(X, C, s)
    assert np.abs(p).max() < 16384.0
    half_ulp = 0.5 * np.spacing(np.abs(p)).astype(np.float64)
    exact = (X.astype(np.int64) - np.array(C)).astype(np.float64) * s
    err = np.abs(p.astype(np.float64) - exact)
    print("frame 'las': max |p - (X - C) s| per axis", err.max(axis=0), "half-ulp bound", half_ulp.max(axis=0))
    assert (err <= half_ulp).all()
    back = p.astype(np.float64) + cw
    literal = np.abs(back - world)
    print("frame 'las': max |(p + centroid_world) - world| per axis", literal.max(axis=0))
    assert (literal <= half_ulp + 1.5 * np.spacing(np.abs(world).max())).all()
    assert np.array_equal(np.rint((back - o) / s).astype(np.int64), X.astype(np.int64))
    # the reference frame on the same rows: float32 cast, float32 sequential mean, float32 centring
    raw = world.astype(np.float32)
    c32 = np.mean(raw, axis=0)
    assert c32.dtype == np.float32
    ref = np.abs((raw - c32).astype(np.float64) + c32.astype(np.float64) - world)
    print("frame 'reference': max error per axis", ref.max(axis=0), "float32 centroid off by",
          np.abs(c32.astype(np.float64) - world.mean(axis=0)))
    assert ref[:, 1].max() > 0.06
    assert literal.max(axis=0)[1] < 1e-4 * ref[:, 1].max()


# ------------------------------------------------------------------ (c) the C ABI
_C_SIZES = {"int64_t": 8, "uint64_t": 8, "double": 8, "float": 4, "int32_t": 4, "uint32_t": 4}


def _header_struct_size(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, align = 0, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        size = _C_SIZES[ctype]
        align = max(align, size)
        for item in names.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\d+)\])?\s*", item)
            off = -(-off // size) * size + size * int(m.group(2) or 1)
    return -(-off // align) * align


def test_frame_abi_host_side():
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    for name in NEW:
        assert name in _lib._SIGS and re.search(r"\b%s\(" % name, header), name
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True)
    assert set(NEW) <= {line.split()[-1] for line in out.stdout.splitlines() if line.strip()}
    assert ctypes.sizeof(_lib.LasFrameC) == _header_struct_size(header, "PchLasFrame") == 80
    assert [f[0] for f in _lib.LasFrameC._fields_] == ["centroid", "count", "count_at_offset", "base", "threshold",
                                                       "aabb", "used_fallback", "reserved"]
    assert _lib.LasFrameC.base.offset == 40 and _lib.LasFrameC.aabb.offset == 48
    assert _lib.LasFrameC.used_fallback.offset == 72
    ws = _lib.lib().pch_ground_filter_las_ws_bytes                 # pure host arithmetic: no device here
    T = ops.FRAME_TILE
    src = open(os.path.join(ROOT, "pointcloudhookup_amd", "csrc", "pch_frame.hip"), encoding="utf-8").read()
    threads, rounds = (int(re.search(r"constexpr int %s\s*= (\d+);" % k, src).group(1)) for k in ("FR_THREADS", "FR_ROUNDS"))
    assert T == threads * rounds                                   # the tile the GPU tests straddle is the kernel's
    ns = [0, 1, 2, T - 1, T, T + 1, 10 * T, 10 ** 6, 10 ** 8, 2 ** 31 - 1]
    got = [ws(n) for n in ns]
    assert got[0] > 0 and all(a <= b for a, b in zip(got, got[1:])) and got[1] < got[7] < got[8]
    assert ws(-1) == 0 and ws(-2 ** 40) == 0
    assert ws(10 ** 8) < 2 * 10 ** 6                               # state, six histograms, two look-back words per tile


# ------------------------------------------------------------------ (d) the knobs
def test_frame_knob_parses(monkeypatch):
    import importlib
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.FRAME == os.environ.get("PCH_FRAME", "reference")
    try:
        monkeypatch.setenv("PCH_FRAME", "las")
        assert importlib.reload(te).FRAME == "las"
        monkeypatch.delenv("PCH_FRAME")
        assert importlib.reload(te).FRAME == "reference"
    finally:
        monkeypatch.undo()
        importlib.reload(te)
    assert pipeline.check_frame("reference", "plane") == "reference" and pipeline.check_frame("las") == "las"
    with pytest.raises(ValueError, match="frame must be"):
        pipeline.check_frame("LAS")


@pytest.mark.parametrize("mode", ["plane", "plane_tiles"])
def test_plane_modes_are_rejected_before_any_device_call(monkeypatch, tmp_path, mode):
    """no device call: the arguments are not even tensors, and the drop-in never reads the (missing) file"""
    with pytest.raises(ValueError, match="percentile ground rule only"):
        pipeline.cluster_points_las(None, (0.001,) * 3, (0.0,) * 3, ground=mode)
    from pointcloudhookup_amd import las
    from pointcloudhookup_amd.utils import tower_extraction as te
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(te, "FRAME", "las")
    monkeypatch.setattr(te, "GROUND_MODE", mode)
    monkeypatch.setattr(las, "read_device", lambda *a: pytest.fail("the file was read"))
    logs = []
    assert te.extract_towers(str(tmp_path / "missing.las"), log_callback=logs.append) == []
    assert logs[:2] == ["📂 读取点云文件...", "🔍 执行高度过滤..."]
    assert len(logs) == 3 and logs[2].startswith("⚠️ 高度过滤失败: ") and "percentile ground rule only" in logs[2]


def test_unknown_frame_is_a_filter_failure(monkeypatch, tmp_path):
    from pointcloudhookup_amd.utils import tower_extraction as te
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(te, "FRAME", "wgs84")
    logs = []
    assert te.extract_towers(str(tmp_path / "missing.las"), log_callback=logs.append) == []
    assert logs[-1].startswith("⚠️ 高度过滤失败: frame must be")


@pytest.mark.parametrize("scales", [(0.001, 0.0, 0.001), (0.001, -0.01, 0.001), (float("nan"), 0.001, 0.001),
                                    (0.001, 0.001, float("inf")), (0.001, 0.001)])
def test_bad_scales_raise_before_any_device_call(scales):
    with pytest.raises(ValueError, match="scales"):
        ops.ground_filter_las(None, scales, (0.0, 0.0, 0.0))
    with pytest.raises(ValueError, match="scales"):
        pipeline.cluster_points_las(None, scales, (0.0, 0.0, 0.0))
