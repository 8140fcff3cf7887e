"""Host side of the many-box crop (pch_crop_boxes_f64): the cull bounds the sweep skips boxes by, the boxes
crop_tower_points builds from tower dicts, and the wrapper's argument errors.  No GPU."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import crop_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _bounds_ctypes(boxes):
    """pch_crop_box_bounds_f64 through ctypes, on a table filled field by field"""
    from pointcloudhookup_amd import _lib
    L = _lib.lib()
    tab = (_lib.CropBoxC * max(len(boxes), 1))()
    for t, b in enumerate(boxes):
        if b[0] == "aabb":
            tab[t].kind = 0
            tab[t].lo[:] = [float(v) for v in b[1]]
            tab[t].hi[:] = [float(v) for v in b[2]]
        else:
            tab[t].kind = 1
            tab[t].center[:] = [float(v) for v in b[1]]
            tab[t].axes[:] = [float(v) for v in np.asarray(b[2]).reshape(9)]
            tab[t].half[:] = [float(v) * 0.5 for v in b[3]]
    out = np.full((len(boxes), 6), -7.0)
    rc = L.pch_crop_box_bounds_f64(C.cast(tab, C.c_void_p), len(boxes), out.ctypes.data)
    return rc, out


def _samples(rng, c, R, h, m):
    """m points around the box (c, R, h): a third uniform in its frame out to 1.5 half extents, a third pushed exactly
    onto faces, edges and corners (frame coordinates of -h, +h), a third a few floats on either side of those"""
    u = rng.uniform(-1.5, 1.5, (m, 3)) * h
    on = rng.integers(0, 3, (m, 3))                          # per axis: 0 free, 1 -> -h, 2 -> +h
    face = np.where(on == 1, -h, np.where(on == 2, h, u))
    k = m // 3
    u[k:2 * k] = face[k:2 * k]
    u[2 * k:] = face[2 * k:] * (1.0 + rng.integers(-4, 5, (m - 2 * k, 3)) * 2.0 ** -52)
    u[-8:] = h * np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])       # the corners
    # world = c + R u, written out (no BLAS)
    return np.stack([c[j] + ((R[j, 0] * u[:, 0] + R[j, 1] * u[:, 1]) + R[j, 2] * u[:, 2]) for j in range(3)], axis=1)


def test_oriented_bounds_hold_every_accepted_point():
    """200 seeded rotations, half extents from 1e-3 to 1e3 (log-uniform per axis), centres at the EPSG-scale offset:
    every one of 20 000 sampled points per box that the predicate accepts lies inside the returned bounds"""
    rng = np.random.default_rng(20250829)
    boxes, samples = [], []
    for t in range(200):
        R = cc.random_rotation(rng) if t >= 5 else cc.named_rotations()[t]
        h = 10.0 ** rng.uniform(-3.0, 3.0, 3)
        c = cc.OFFSET + rng.uniform(-500.0, 500.0, 3)
        boxes.append(("obb", c, R, 2.0 * h))
        samples.append(_samples(rng, c, R, h, 20000))
    rc, bounds = _bounds_ctypes(boxes)
    assert rc == 0 and np.isfinite(bounds).all()
    accepted = 0
    for b, P, bd in zip(boxes, samples, bounds):
        m = cc.inside(P, b)
        accepted += int(m.sum())
        Q = P[m]
        assert (Q >= bd[None, :3]).all() and (Q <= bd[None, 3:]).all()
        # and they are bounds of the box, not of the world: within 1e-5 of the widest half extent of the exact ones
        r = np.abs(b[2]) @ (b[3] * 0.5)
        assert (np.abs((bd[3:] - bd[:3]) * 0.5 - r) <= 1e-5 * (b[3] * 0.5).max() + 1e-8).all()
    assert accepted > 200 * 20000 // 12                      # the samples do test something


def test_axis_aligned_bounds_are_the_box():
    boxes = [b for b in cc.special_boxes() if b[0] == "aabb"]
    rc, bounds = _bounds_ctypes(boxes)
    assert rc == 0
    for b, bd in zip(boxes, bounds):
        np.testing.assert_array_equal(bd[:3], b[1])           # NaN and inf included, bit for bit
        np.testing.assert_array_equal(bd[3:], b[2])


def test_bounds_of_boxes_with_nan_or_inf_fields_are_not_finite():
    """the call succeeds; bounds that are not all finite mean `never skipped` (the GPU test shows they are not)"""
    sp = cc.special_boxes()
    odd = [b for b in sp if b[0] == "obb" and not (np.isfinite(b[1]).all() and np.isfinite(b[2]).all()
                                                   and np.isfinite(b[3]).all())]
    assert len(odd) == 3
    skew = [b for b in sp if b[0] == "obb" and np.isfinite(b[2]).all()
            and np.abs(np.asarray(b[2]).T @ np.asarray(b[2]) - np.eye(3)).max() > 1e-3]
    assert len(skew) == 1
    rc, bounds = _bounds_ctypes(odd + skew)
    assert rc == 0
    assert not np.isfinite(bounds).all(axis=1).any()
    from pointcloudhookup_amd import ops
    np.testing.assert_array_equal(ops.crop_box_bounds(odd + skew), bounds)       # the wrapper's table is the same


def test_bounds_reject_bad_tables():
    from pointcloudhookup_amd import _lib
    L = _lib.lib()
    tab = (_lib.CropBoxC * 2)()
    tab[1].kind = 2
    out = np.zeros((2, 6))
    assert L.pch_crop_box_bounds_f64(C.cast(tab, C.c_void_p), 2, out.ctypes.data) == -1       # PCH_ERR_ARG
    assert L.pch_crop_box_bounds_f64(C.cast(tab, C.c_void_p), 4097, out.ctypes.data) == -1
    assert L.pch_crop_box_bounds_f64(None, 0, None) == 0
    assert L.pch_crop_boxes_ws_bytes(1000, 3, 100) > 0 and L.pch_crop_boxes_ws_bytes(1000, 4097, 100) == 0


# ------------------------------------------------------------------ the boxes of crop_tower_points
def test_tower_boxes_kuangxuan_presets_equal_the_golden_boxes():
    from pointcloudhookup_amd.ui import extract as ex
    g = json.load(open(os.path.join(GOLD, "kuangxuan_boxes.json")))
    tower = dict(center=np.array(g["center"]), extent=np.array(g["extent"]), rotation=np.eye(3))
    for preset, ref in g["presets"].items():
        (box,) = ex.tower_crop_boxes([tower], kuangxuan_preset=preset)
        assert box[0] == "aabb"
        np.testing.assert_allclose(box[1], ref["min"], atol=5e-3)     # the golden file's own rounding (test_host.py)
        np.testing.assert_allclose(box[2], ref["max"], atol=5e-3)
        lo, hi = ex.create_bbox_using_kuangxuan_method(tower["center"], 20.1, 17.4, **ex.get_bbox_preset(preset)[1])
        np.testing.assert_array_equal(box[1], lo)
        np.testing.assert_array_equal(box[2], hi)
    assert len(g["presets"]) == 3
    # a symmetric preset: the box _bounds_for gives
    (box,) = ex.tower_crop_boxes([tower], kuangxuan_preset="symmetric_large")
    lo, hi = ex._bounds_for(tower["center"], 20.1, 17.4, *ex.get_bbox_preset("symmetric_large"))
    assert box[0] == "aabb"
    np.testing.assert_array_equal(box[1], lo)
    np.testing.assert_array_equal(box[2], hi)


def test_tower_boxes_oriented_branch_uses_the_drawn_scales(capsys, monkeypatch):
    """three heights, one in each band of the adaptive table: the box is the one extract_and_visualize_towers_original
    draws - its 24 line points are the corners of (center, rotation, extent * scale)"""
    from pointcloudhookup_amd.ui import extract as ex
    R = cc.rot_z(30.0)
    towers = [dict(center=cc.OFFSET + [10.0 * k, 5.0, 2.0], rotation=R, extent=np.array([6.0, 8.0, h]))
              for k, h in enumerate((12.0, 25.0, 47.0))]
    want = ([3.2, 3.2, 5.0], [3.0, 3.0, 4.8], [2.8, 2.8, 4.5])
    boxes = ex.tower_crop_boxes(towers, use_kuangxuan_method=False)
    for tw, box, sc in zip(towers, boxes, want):
        assert box[0] == "obb" and ex._adaptive_scale(tw["extent"][2]) == sc
        np.testing.assert_array_equal(box[1], tw["center"])
        np.testing.assert_array_equal(box[2], R)
        np.testing.assert_array_equal(box[3], tw["extent"] * np.array(sc))
        np.testing.assert_array_equal(ex._obb_line_points(box[1], box[2], box[3]),
                                      ex._obb_line_points(tw["center"], R, tw["extent"] * np.array(sc)))
    fixed = ex.tower_crop_boxes(towers, scale_factors=[2.0, 3.0, 4.0], adaptive_scaling=False,
                                use_kuangxuan_method=False)
    for tw, box in zip(towers, fixed):
        np.testing.assert_array_equal(box[3], tw["extent"] * np.array([2.0, 3.0, 4.0]))
    # what the drawing function draws with the same arguments (its cloud read stubbed out: no GPU here)
    monkeypatch.setattr(ex, "_read_cloud", lambda path: np.zeros((0, 3)))
    for kw, bx in ((dict(), boxes), (dict(scale_factors=[2.0, 3.0, 4.0], adaptive_scaling=False), fixed)):
        drawn = ex.extract_and_visualize_towers("unused.las", towers, use_kuangxuan_method=False, **kw)[1]
        assert len(drawn) == 3
        for (pts, _), box in zip(drawn, bx):
            np.testing.assert_array_equal(pts, ex._obb_line_points(box[1], box[2], box[3]))
    # a malformed dict: None (an empty result later) and a printed warning, the good ones unharmed
    capsys.readouterr()
    mixed = ex.tower_crop_boxes([towers[0], dict(center=towers[0]["center"]), towers[1]], use_kuangxuan_method=False)
    assert mixed[1] is None and mixed[0] is not None and mixed[2] is not None
    assert "⚠️" in capsys.readouterr().out
    assert ex.tower_crop_boxes([dict(extent=[1, 2, 3])])[0] is None


def test_crop_tower_points_missing_file():
    from pointcloudhookup_amd.ui import extract as ex
    with pytest.raises(FileNotFoundError, match="未找到文件"):
        ex.crop_tower_points("/nonexistent/file.las", [])


# ------------------------------------------------------------------ argument errors of the wrapper
def test_wrapper_argument_errors():
    import torch
    from pointcloudhookup_amd import ops
    xyz = torch.zeros((10, 3), dtype=torch.float64)
    one = ("aabb", [0.0] * 3, [1.0] * 3)
    with pytest.raises(ValueError, match="4096"):
        ops.crop_boxes(xyz, [one] * 4097)
    with pytest.raises(ValueError, match="kind"):
        ops.crop_boxes(xyz, [one, ("sphere", [0.0] * 3, 1.0)])
    tab = ops.crop_box_table([one, one])
    tab["kind"][1] = 7
    with pytest.raises(ValueError, match="kind"):
        ops.crop_boxes(xyz, tab)
    with pytest.raises(ValueError, match="float64"):
        ops.crop_boxes(xyz.to(torch.float32), [one])
    with pytest.raises(ValueError):
        ops.crop_boxes(xyz, [("obb", [0.0] * 3, np.eye(2), [1.0] * 3)])
    with pytest.raises(TypeError, match="no CPU fallback"):               # like every other ops.*
        ops.crop_boxes(xyz, [one])
    # the table of a list and a prepared table are the same records
    t2 = ops.crop_box_table([one, ("obb", [1.0, 2.0, 3.0], cc.rot_z(30.0), [2.0, 4.0, 6.0])])
    assert t2.dtype.itemsize == 176 and list(t2["kind"]) == [0, 1]
    np.testing.assert_array_equal(t2["half"][1], [1.0, 2.0, 3.0])
    np.testing.assert_array_equal(t2["axes"][1], cc.rot_z(30.0).reshape(9))
    assert ops.crop_box_table(t2) is t2 or (ops.crop_box_table(t2) == t2).all()
