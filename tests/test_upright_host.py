"""The upright boxes of stage D1 without a GPU: the numpy statement of tests/upright_cases.py checked against its own
construction and the derived quality bound, pipeline.upright_boxes_from_records against the statement's
tower_from_record, the end-to-end cloud through the accept rule, and the symbols of the C ABI."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import merge_cases as mc
import upright_cases as uc
from pointcloudhookup_amd import pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = uc.rectangles()
DEFAULTS = (0.8, 15.0, 50.0, 8, 30.0)        # aspect_ratio_threshold, min_height, max_width, min_width, duplicate_threshold


@functools.lru_cache(maxsize=None)
def _box(name, exact=False):
    return uc.box(CASES[name]["exact" if exact else "rows"])


# ------------------------------------------------------------------------------------------- the statement on itself
@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["index"] is not None and CASES[n]["aspect"] != 1.0])
def test_on_table_rectangles_are_found(name):
    """the optimum lies on a table index: that index is j.  On the rows as constructed (float64) du, dv are 20 and 8 to
    1e-9; on their float32 roundings - coordinates below 16 m, so each moves by at most 2^-21 m (half an ulp of 8..16),
    a projection by at most sqrt(2) times that and a width by twice that, 1.35e-6 - to 1.5e-6"""
    want = CASES[name]["index"]
    for exact, tol in ((True, 1e-9), (False, 1.5e-6)):
        rec, _ = _box(name, exact)
        assert rec["status"] == 0 and rec["j"] == want
        assert rec["j0"] == want if want % uc.FINE == 0 else abs(int(rec["j0"]) - want) < uc.FINE
        du, dv = rec["umax"] - rec["umin"], rec["vmax"] - rec["vmin"]
        assert abs(du - 20.0) <= tol and abs(dv - 8.0) <= tol, (du, dv)


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n]["area"] is not None])
def test_derived_bound_holds(name):
    case = CASES[name]
    rec, area0 = _box(name)
    area1 = float(uc.area_of(rec))
    print(name, "j0", rec["j0"], "j", rec["j"], "area0", area0, "area1", area1, "true", case["area"])
    assert area1 <= case["area"] * uc.bound_factor(case["aspect"]) * (1 + 1e-12)
    assert area1 <= area0


@pytest.mark.parametrize("name", list(CASES))
def test_level_1_never_loses_to_level_0(name):
    rec, area0 = _box(name)
    assert float(uc.area_of(rec)) <= area0
    assert rec["j0"] % uc.FINE == 0 and min((rec["j"] - rec["j0"]) % uc.T, (rec["j0"] - rec["j"]) % uc.T) < uc.FINE


def test_ties_and_zero_areas_go_to_the_smallest_index():
    for name in ("single_point", "same_point_twice"):
        rec, area0 = _box(name)
        assert rec["j"] == 0 and rec["j0"] == 0 and area0 == 0.0 and rec["umin"] == rec["umax"]
    rec, _ = _box("two_points")                          # along x: zero area at index 0 only
    assert rec["j"] == 0 and rec["vmin"] == rec["vmax"] == 2.0 and (rec["umin"], rec["umax"]) == (1.0, 6.0)
    rec, _ = _box("collinear_y")
    assert rec["j"] == 0 and rec["umin"] == rec["umax"] == 2.0
    rec, _ = _box("square")
    assert rec["j"] == 0 and rec["umax"] - rec["umin"] == 6.0 and rec["vmax"] - rec["vmin"] == 6.0
    rec, _ = _box("wrap_89.99")
    assert rec["j0"] == 0
    rec, _ = _box("wrap_89.97")
    assert rec["j0"] == 0 and rec["j"] == uc.T - 1


def test_status_1_records():
    for rows in (np.zeros((0, 3), np.float32), np.array([[0, 0, 0], [1, np.nan, 2]], np.float32),
                 np.array([[0, 0, np.inf]], np.float32), np.array([[-np.inf, 0, 0]], np.float32)):
        rec, _ = uc.box(rows)
        assert rec["status"] == 1 and rec["j"] == -1 and rec["j0"] == -1 and rec["n"] == len(rows)
        assert all(np.isnan(rec[f]) for f in uc.BOUNDS)
        assert uc.tower_from_record(rec) is None


# -------------------------------------------------------------------------- records -> boxes, against the statement
def _all_records():
    P, lab, K = uc.centers_cloud("mixed_sign")
    recs = [uc.expected(P, lab, K)]
    recs.append(np.array([_box(name)[0] for name in CASES], dtype=uc.RECORD))
    return np.concatenate(recs)


def test_boxes_from_records_equal_the_statement():
    records = _all_records()
    boxes = pipeline.upright_boxes_from_records(records)
    assert len(boxes) == len(records) and (records["status"] == 1).sum() == 3
    cs = uc.table()
    for rec, (box, err) in zip(records, boxes):
        want = uc.tower_from_record(rec, cs)
        if want is None:
            assert box is None and isinstance(err, ValueError)
            continue
        assert err is None
        extents, transform = box
        assert isinstance(extents, np.ndarray) and extents.dtype == np.float64 and transform.shape == (4, 4)
        np.testing.assert_array_equal(extents, want[0])
        np.testing.assert_array_equal(transform, want[1])
        R = transform[:3, :3]
        np.testing.assert_allclose(R.T @ R, np.eye(3), atol=1e-15)
        assert abs(np.linalg.det(R) - 1.0) < 1e-15 and R[:, 2].tolist() == [0.0, 0.0, 1.0]
        assert extents[0] >= extents[1] and extents[2] == rec["zmax"] - rec["zmin"]
        assert transform[3].tolist() == [0.0, 0.0, 0.0, 1.0]


def test_zero_width_is_a_warning_not_an_exception():
    """a pole: height 20 over a footprint of one point, so the aspect ratio is 20 / 0 = inf in numpy float64"""
    rec, _ = uc.box(np.array([[1.0, 1.0, 0.0], [1.0, 1.0, 20.0]], dtype=np.float32))
    boxes = pipeline.upright_boxes_from_records(np.array([rec], dtype=uc.RECORD))
    assert boxes[0][0][0].tolist() == [0.0, 0.0, 20.0]
    with pytest.warns(RuntimeWarning, match="divide by zero"):
        events = pipeline._accept(boxes, np.zeros(3, np.float32), *DEFAULTS)
    assert events == []                                  # not a failure line either: the width rule rejects it


# ---------------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def e2e_statement():
    """(filtered rows, tower id per row, records of the four true towers, centroid) by the CPU oracle's filter"""
    from oracle import ground_filter as ogf
    raw, tower = mc.e2e_cloud()
    g = ogf.ground_filter(raw)
    who = tower[g["keep"]]
    return g["filtered"], who, uc.expected(g["filtered"], who, 4), g["centroid"]


def test_e2e_towers_pass_the_default_accept_rule():
    rows, who, records, centroid = e2e_statement()
    assert records["n"].tolist() == mc.E2E_TOWERS and not records["status"].any()
    events = pipeline._accept(pipeline.upright_boxes_from_records(records), centroid, *DEFAULTS)
    towers = [t for kind, t in events if kind == "tower"]
    assert [kind for kind, _ in events] == ["tower"] * 4 and [t["label"] for t in towers] == [0, 1, 2, 3]
    for t, rec in zip(towers, records):
        z = rows[who == t["label"], 2]
        assert t["height"] == np.float64(z.max()) - np.float64(z.min()) == rec["zmax"] - rec["zmin"]
        print(t["label"], "extent", t["extent"], "aspect", t["aspect_ratio"], "north", t["north_angle"])
        assert 8 < t["width"] < 50 and t["height"] > 15 and t["aspect_ratio"] >= 2.38
        assert t["width"] == t["extent"][0] >= t["extent"][1]


# ------------------------------------------------------------------------------------------------------- symbols
def test_symbols_and_workspace_size():
    from pointcloudhookup_amd import _lib
    header = open(os.path.join(ROOT, "include", "pch_hip.h")).read()
    for name in ("pch_upright_boxes_f32", "pch_upright_boxes_ws_bytes"):
        assert name in _lib._SIGS and re.search(r"\b" + name + r"\s*\(", header)
    assert re.search(r"#define\s+PCH_UPRIGHT_COARSE\s+128\b", header) and re.search(r"#define\s+PCH_UPRIGHT_FINE\s+32\b", header)
    assert ctypes.sizeof(_lib.UprightBoxC) == 72 == uc.RECORD.itemsize
    assert [(n, uc.RECORD.fields[n][1]) for n in uc.RECORD.names] == \
        [(n, getattr(_lib.UprightBoxC, n).offset) for n, _ in _lib.UprightBoxC._fields_]
    ws = _lib.lib().pch_upright_boxes_ws_bytes
    ks = [1, 2, 3, 4, 5, 7, 63, 64, 65, 200, 201, 4095, 4096, 4097, 16383, 16384, 16385, 65536, 1_000_000]
    caps = [0, 1, 255, 256, 257, 4096, 65_536, 300_001, 10_000_000, 2_000_000_000]
    size = np.array([[ws(k, cap) for cap in caps] for k in ks], dtype=np.float64)
    assert (size > 0).all() and ws(0, 1000) == 0
    assert (np.diff(size, axis=0) >= 0).all() and (np.diff(size, axis=1) >= 0).all()
    assert size[ks.index(16384), -1] <= 80 << 20         # a bounded table, not clusters x tiles
