"""Span sections on the CPU: the numpy statement of the rule (section_cases) against an independent statement in space
and against hand-set boundary rows, the float32 cast against the order of the doubles, the drop-in's knob and csv
writer, the new symbols, the workspace size and the header's lines (no kernel runs here)."""
import csv
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import section_cases as sn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pch_span_section_ws_bytes", "pch_span_section_f32")


def test_the_rule_against_the_statement_in_space():
    """random sloped spans, three parallel phases among them: away from every decision (1e-6 m) the strip-and-parabola
    statement gives the rule's cells, stations and per-row answers; the distances agree to float32's rounding"""
    checked = 0
    for n, K, B, seed in ((3000, 9, 16, 1), (2000, 12, 64, 2), (1500, 3, 128, 3), (800, 5, 1, 4)):
        X, C = sn.random_case(n, K, seed, phases=seed == 2)
        half, depth, limit = 12.0, 25.0, 6.0
        brute = [sn.strip_brute(X, c, B, half, depth, limit) for c in C]
        margin = np.minimum.reduce([b["margin"] for b in brute])
        skip = (margin < 1e-6).astype(np.uint8)
        assert skip.sum() < n // 100
        ref = sn.section_reference(X, C, B, half, depth, limit, skip=skip)
        alive = skip == 0
        best = np.full(n, np.inf)
        who = np.full(n, -1)
        for k, b in enumerate(brute):
            part = b["part"] & alive
            count = np.bincount(b["j"][part], minlength=B)
            viol = np.bincount(b["j"][b["viol"] & alive], minlength=B)
            assert np.array_equal(count, ref["count"][k]) and np.array_equal(viol, ref["violations"][k]), (seed, k)
            for j in np.flatnonzero(count):
                rows = np.flatnonzero(part & (b["j"] == j))
                lowest = b["v"][rows].min()
                assert abs(float(ref["min_v"][k, j]) - lowest) <= 4e-6 + 1e-9   # 2^-24 * depth, and the statement's own
                assert ref["min_row"][k, j] in rows and b["v"][ref["min_row"][k, j]] <= lowest + 8e-6
            assert np.isinf(ref["min_v"][k][count == 0]).all() and (ref["min_row"][k][count == 0] == -1).all()
            closer = part & (b["v"] < best - 1e-5)
            best = np.where(part, np.minimum(best, b["v"]), best)
            who = np.where(closer, k, who)
            checked += int(part.sum())
        hit = np.isfinite(best)
        assert np.array_equal(hit, ref["span"] >= 0) and np.array_equal(hit, ref["station"] >= 0)
        assert np.abs(ref["v"][hit].astype(np.float64) - best[hit]).max() <= 4e-6 + 1e-9
        for i in np.flatnonzero(hit):
            k = ref["span"][i]
            assert brute[k]["part"][i] and brute[k]["v"][i] <= best[i] + 8e-6 and ref["station"][i] == brute[k]["j"][i]
        if seed == 2:                                                          # under three phases: counted in all three
            many = sum((b["part"] & alive).astype(int) for b in brute)
            assert (many >= 3).sum() > 100 and ref["count"].sum() == many.sum()
    assert checked > 3000


def test_the_boundary_rows_by_hand():
    X, skip, curves, want = sn.edge_case()
    assert sn.takes_part(curves).tolist() == [False, True, True]
    ref = sn.section_reference(X, curves, sn.E_STATIONS, sn.E_HALF, sn.E_DEPTH, sn.E_LIMIT, skip=skip)
    part = np.array([w[0] for w in want])
    station = np.array([w[1] for w in want])
    viol = np.array([w[2] for w in want])
    assert np.array_equal(ref["span"], np.where(part, 1, -1)) and np.array_equal(ref["station"], station)
    assert np.array_equal(np.isfinite(ref["v"]), part)
    for k in (1, 2):                                                           # the second wire sees the same rows
        assert np.array_equal(ref["count"][k], np.bincount(station[part], minlength=4))
        assert np.array_equal(ref["violations"][k], np.bincount(station[viol], minlength=4))
    assert ref["count"][0].sum() == 0 and np.isinf(ref["min_v"][0]).all() and (ref["min_row"][0] == -1).all()
    assert ref["v"][14] == 0.0 and ref["v"][17] == 4.0 and ref["v"][20] == 16.0 and ref["v"][0] == 8.0
    assert ref["min_v"][1].tolist() == [1.0, 6.0, 0.0, 0.5] and ref["min_row"][1].tolist() == [29, 8, 14, 30]
    # v just above the limit rounds to the limit in float32 or not: the violation is decided on the double either way
    assert ref["v"][18] >= np.float32(4.0) and not viol[18]


def test_the_cast_never_reorders_a_minimum():
    """fabsf((float)v) is monotone: for doubles a <= b the casts satisfy fa <= fb, so the smallest cast is the cast of
    the smallest double - on neighbours, on ties of the cast and on random values"""
    rng = np.random.default_rng(8)
    v = np.concatenate([rng.uniform(0.0, 80.0, 200000), np.float64(np.float32(rng.uniform(0.0, 80.0, 1000))),
                        [0.0, 5e-324, 2.0 ** -149, 2.0 ** -150, 2.0 ** -126, 80.0]])
    v = np.concatenate([v, np.nextafter(v, np.inf), np.nextafter(v, 0.0)])
    v.sort()
    f = np.abs(v.astype(np.float32))
    assert (np.diff(f) >= 0).all() and (f.view(np.uint32)[1:] >= f.view(np.uint32)[:-1]).all()
    assert (np.diff(f) == 0).sum() > 1000                                      # ties of the cast exist
    for lo in range(0, len(v) - 64, 997):
        assert np.abs(v[lo:lo + 64].astype(np.float32)).min() == np.abs(np.float32(v[lo:lo + 64].min()))
    # non-negative float32 bit patterns order as unsigned integers, and all ones is above every one of them
    keys = (f.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(7)
    assert (np.diff(keys.astype(np.float64)) >= 0).all() and keys.max() < np.uint64(2 ** 64 - 1)


def test_knob_parser_and_the_csv_writer(tmp_path):
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.section_from_env(None) is None and te.section_from_env("  ") is None
    assert te.section_from_env(None, spans=False) is None                    # off needs nothing
    assert te.section_from_env("15, 7") == dict(half_width=15.0, limit=7.0, stations=64, depth=80.0)
    assert te.section_from_env("15,7,32") == dict(half_width=15.0, limit=7.0, stations=32, depth=80.0)
    assert te.section_from_env("15,7,64,80") == dict(half_width=15.0, limit=7.0, stations=64, depth=80.0)
    assert te.section_from_env("5,30,128,30")["depth"] == 30.0
    for bad in ("15", "15,7,64,80,1", "0,7", "-1,7", "nan,7", "inf,7", "15,0", "15,-1", "15,81", "15,7,0", "15,7,129",
                "15,7,64,5", "15,7,64,inf", "15,nan", "15,7,1.5", "a,b"):
        with pytest.raises(ValueError):
            te.section_from_env(bad)
    with pytest.raises(ValueError, match="PCH_SPANS"):
        te.section_from_env("15,7", spans=False)
    assert te.SECTION is None or te.SPANS is not None
    assert te.SECTION_COLUMNS == ("ID", "station", "m", "x", "y", "wire_z", "ground_z", "count", "violations",
                                  "min_vertical", "min_row", "top_x", "top_y", "top_z")
    nan, inf = float("nan"), float("inf")
    section = dict(pieces=torch.tensor([2]), m=torch.tensor([[-10.0, 10.0]], dtype=torch.float64),
                   xy=torch.tensor([[[1.0, 2.0], [3.0, 4.0]]], dtype=torch.float64),
                   wire_z=torch.tensor([[20.0, 21.0]], dtype=torch.float64),
                   ground=torch.tensor([[nan, 0.5]], dtype=torch.float64), count=torch.tensor([[0, 5]]),
                   violations=torch.tensor([[0, 2]]), min_vertical=torch.tensor([[inf, 3.25]], dtype=torch.float32),
                   min_row=torch.tensor([[-1, 9]]),
                   top=torch.tensor([[[nan] * 3, [3.5, 4.5, 17.75]]], dtype=torch.float32))
    rows = te.section_rows(section, np.array([100.0, 200.0, 300.0]))
    assert rows[1] == ["span_2", 1, 10.0, 103.0, 204.0, 321.0, 300.5, 5, 2, 3.25, 9, 103.5, 204.5, 317.75]
    assert rows[0][:6] == ["span_2", 0, -10.0, 101.0, 202.0, 320.0] and rows[0][7:9] == [0, 0]
    path = tmp_path / "section_info.csv"
    te.write_section_csv(path, rows)
    with open(path, newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == te.SECTION_COLUMNS and len(lines) == 3
    assert lines[2] == ["span_2", "1", "10.0", "103.0", "204.0", "321.0", "300.5", "5", "2", "3.25", "9", "103.5",
                        "204.5", "317.75"]
    assert lines[1][6] == "nan" and lines[1][9] == "inf" and lines[1][10] == "-1" and lines[1][11] == "nan"
    line = te.section_line(section, rows, te.section_from_env("15,7"))
    assert "导线断面" in line and "越限区段 1/2" in line and "3.250 m" in line


def test_knob_without_the_span_knob_fails_at_import():
    env = {k: v for k, v in os.environ.items() if k not in ("PCH_SPANS", "PCH_SECTION")}
    code = "import pointcloudhookup_amd.utils.tower_extraction as te; print(te.SECTION)"
    bad = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, PCH_SECTION="15,7"), capture_output=True,
                         text=True)
    assert bad.returncode != 0 and "ValueError" in bad.stderr and "PCH_SPANS" in bad.stderr
    good = subprocess.run([sys.executable, "-c", code], cwd=ROOT,
                          env=dict(env, PCH_SECTION="15,7,32", PCH_SPANS="1,5,9,20"), capture_output=True, text=True)
    assert good.returncode == 0 and "'stations': 32" in good.stdout, good.stderr


def test_new_symbols_workspace_bytes_and_the_header():
    from pointcloudhookup_amd import _lib, ops, pipeline
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(pch_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    L = _lib.lib()
    ws = L.pch_span_section_ws_bytes
    assert ws(0, 0, 1) > 0 and ws(0, 0, 1) == ws(10 ** 8, 1, 128)            # per span, not per row or cell
    assert ws(0, 4096, 128) > ws(0, 1, 128) and ws(2 ** 32 - 1, 4096, 128) == ws(0, 4096, 1)
    assert ws(0, 4096, 128) <= 4096 * 64
    for n, K, B in ((-1, 1, 1), (2 ** 32, 1, 1), (1, -1, 1), (1, 4097, 1), (1, 1, 0), (1, 1, 129)):
        assert ws(n, K, B) == 0, (n, K, B)
    assert ops.SECTION_MAX_STATIONS == 128 and callable(ops.span_section) and callable(pipeline.span_sections)
    for bad in (0, 129, 1.5, True):
        with pytest.raises(ValueError):
            ops.check_stations(bad)
    assert ops.check_stations(64.0) == 64
    at = header.index("span sections, opt-in (DESIGN.md 5j)")
    rule = header[at:header.index("pch_span_section_f32(", header.index("size_t pch_span_section_ws_bytes", at))]
    for line in ("dx = (double)px - cx;  dy = (double)py - cy;  w = (double)pz - cz",
                 "m = (dx*ux) + (dy*uy);  t = (dy*ux) - (dx*uy)",
                 "in the corridor iff  m >= m0 and m <= m1 and t >= -half and t <= half",
                 "zw = a + (m*(b + (c*m)));  v = zw - w", "takes part iff in the corridor and v >= 0.0 and v <= depth",
                 "j = (int)floor((m - m0) / step);  if j > B - 1: j = B - 1", "vf = fabsf((float)v)",
                 "step = (m1 - m0) / (double)B", "chord_error", "not the nearest-only attribution", "EVERY row"):
        assert line in rule, line


def test_the_pipeline_and_the_op_refuse_a_cpu_tensor():
    from pointcloudhookup_amd import ops, pipeline
    X = torch.zeros((4, 3), dtype=torch.float32)
    with pytest.raises(TypeError):
        pipeline.span_sections(X, {})
    with pytest.raises(TypeError):
        pipeline.span_sections(X.numpy(), {})
    with pytest.raises(TypeError):
        ops.span_section(X, torch.zeros((1, 10), dtype=torch.float64), 4, 15.0, 80.0, 7.0)
