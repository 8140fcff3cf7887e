"""Tower profile on the CPU: the new symbols and workspace sizes, the two numpy statements of the slice table against
each other, ``ops._tower_levels_of`` on CPU tensors against ``levels_reference``, the scene's numbers and margins, the
drop-in's knob and the header's lines (no kernel runs here)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import span_cases as sp
import terrain_cases as tc
import tower_profile_cases as tp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pch_cluster_slices_ws_bytes", "pch_cluster_slices_f32")


def test_new_symbols_and_workspace_bytes():
    from pointcloudhookup_amd import _lib, ops, pipeline
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    declared = set(re.findall(r"\b(pch_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    ws = _lib.lib().pch_cluster_slices_ws_bytes
    # four 64-bit keys per (table, slice), whatever the rows and the clusters
    assert ws(0, 0, 1, 1) > 0 and ws(0, 0, 3, 128) == ws(2 ** 31 - 1, 2 ** 31 - 1, 3, 128)
    assert 32 * 3 * 128 <= ws(1000, 5, 3, 128) <= 32 * 3 * 128 + 1024
    assert 32 * 2 ** 20 <= ws(1, 1, 4096, 256) <= 32 * 2 ** 20 + 1024
    for n, K, T, B in ((-1, 1, 1, 1), (2 ** 31, 1, 1, 1), (1, -1, 1, 1), (1, 1, 0, 1), (1, 1, -1, 1), (1, 1, 4097, 1),
                       (1, 1, 1, 0), (1, 1, 1, -1), (1, 1, 1, 257), (1, 1, 4097, 256)):
        assert ws(n, K, T, B) == 0, (n, K, T, B)
    assert (ops.SLICES_BLOCK, ops.SLICES_MAX, ops.SLICES_MAX_TABLES) == (512, 256, 4096)
    for name in ("cluster_slices", "tower_levels", "_tower_levels_of"):
        assert callable(getattr(ops, name)), name
    assert callable(pipeline.tower_profile)
    assert pipeline.TOWER_PROFILE_TABLE_KEYS == ("ground", "ground_from", "top", "tower_height", "nominal_height",
                                                 "n_levels", "z_low", "z_high", "width", "rows", "lowest_wire")


def test_the_header_carries_the_rule():
    header = open(os.path.join(ROOT, "include", "pch_hip.h"), encoding="utf-8").read()
    for line in ("frames5[k] = (cx, cy, z0, ux, uy)",
                 "Cluster k takes part iff 0 <= slot[k] < T and all five frame values are finite.",
                 "dx = (double)px - cx;  dy = (double)py - cy;  h = (double)pz - z0",
                 "s = (dx*ux) + (dy*uy);  t = (dy*ux) - (dx*uy);  q = floor(h / dz)",
                 "If q < 0: out_outside[slot,0] += 1.", "If q >= B: out_outside[slot,1] += 1.",
                 "A NaN q counts nowhere.",
                 "The row is binned iff 0 <= q < B and s and t are finite, with b = (int)q.",
                 "out_ext[slot,b] = (min s, max s, min t, max t)", "-0.0 sorts below +0.0",
                 "A slice without a row holds (+inf, -inf, +inf, -inf) and count 0.",
                 "Clusters that share a slot are combined as if they were one.",
                 "0 <= n_grouped < 2^31, nclusters >= 0, 1 <= T <= 4096, 1 <= B <= 256, T*B <= 2^20, dz finite and > 0",
                 "A refused call writes nothing.", "arm[b] = occ[b] and (w[b] - body[b]) >= arm_excess",
                 "An arm thicker than 2G + 1 slices is not found."):
        assert line in header, line


# ------------------------------------------------------------------ the two statements
def _awkward_case(n, K, T, seed):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(-3, 20, n)], axis=1).astype(np.float32)
    on = rng.uniform(0, 1, n) < 0.2
    X[on, 2] = np.round(X[on, 2] * 2) / 2                                   # rows on slice boundaries
    for k, v in enumerate((np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf)):
        X[(7 * k + 3) % n, k % 3] = v
    X[rng.integers(0, n, n // 10), 0] = np.float32(-0.0)
    X[rng.integers(0, n, n // 10), 1] = np.float32(0.0)
    perm = rng.permutation(n).astype(np.int32)
    offsets = np.concatenate([[0], np.sort(rng.integers(0, n - 20, K - 1)), [n - 20]]).astype(np.int64)
    th = rng.uniform(0, np.pi, K)
    frames5 = np.stack([np.zeros(K), np.zeros(K), rng.choice([-3.0, 0.0, 0.5], K), np.cos(th), np.sin(th)], axis=1)
    frames5[0, 3:5] = (1.0, 0.0)
    slot = rng.integers(-1, T + 1, K).astype(np.int32)
    return X, perm, offsets, frames5, slot


@pytest.mark.parametrize("K,T,B", [(1, 1, 1), (3, 2, 2), (7, 3, 40), (65, 5, 256)])
def test_slice_table_by_a_loop_and_by_a_sort(K, T, B):
    X, perm, offsets, frames5, slot = _awkward_case(1500, K, T, seed=K)
    a = tp.slices_reference(X, perm, offsets, frames5, slot, T, 0.5, B)
    b = tp.slices_by_sort(X, perm, offsets, frames5, slot, T, 0.5, B)
    for name, u, v in zip(("count", "ext", "outside"), a, b):
        assert u.dtype == v.dtype and np.array_equal(u.view(np.uint8), v.view(np.uint8)), name
    part = tp.takes_part(frames5, slot, T)
    rows = sum(int(offsets[k + 1] - offsets[k]) for k in range(K) if part[k])
    assert a[0].sum() + a[2].sum() <= rows and (a[1][a[0] == 0] == np.array(tp.EMPTY)).all()
    assert np.isfinite(a[1][a[0] > 0]).all()
    assert np.array_equal(tp.unkey64(tp.key64(X[:, 0].astype(np.float64))).view(np.uint64),
                          X[:, 0].astype(np.float64).view(np.uint64))
    assert tp.key64(np.array([-0.0]))[0] < tp.key64(np.array([0.0]))[0]


# ------------------------------------------------------------------ levels
def _table(widths, counts=None):
    """count [1,B] and ext [1,B,4] of a tower whose slice b is widths[b] wide along s (0 or None: an empty slice)"""
    B = len(widths)
    count = np.zeros((1, B), dtype=np.int32)
    ext = np.empty((1, B, 4))
    ext[:] = tp.EMPTY
    for b, w in enumerate(widths):
        if w:
            count[0, b] = 10 if counts is None else counts[b]
            ext[0, b] = (-0.5 * w, 0.5 * w, -0.25 * w, 0.125 * w)
    return count, ext


def _levels_agree(count, ext, z0, dz, ground=None, **kw):
    from pointcloudhookup_amd import ops
    want = tp.levels_reference(count, ext, z0, dz, ground=ground, **kw)
    T = count.shape[0]
    col = lambda v: None if v is None else torch.from_numpy(np.broadcast_to(np.asarray(v, dtype=np.float64), (T,)).copy())
    got = ops._tower_levels_of(torch.from_numpy(count), torch.from_numpy(ext), col(z0), dz, col(ground), **kw)
    assert set(got) == set(want)
    for key in want:
        g = got[key].numpy()
        assert g.dtype == want[key].dtype and tc.same(g, want[key]), (key, g, want[key])
    return want


def test_levels_on_the_cases_of_the_rule():
    body = [3.0] * 12
    kw = dict(min_rows=3, arm_window=1.5, arm_excess=4.0, max_levels=8)       # dz 0.5: G = 3, 2G + 1 = 7
    none = _levels_agree(*_table([0] * 12), 1.0, 0.5, ground=0.25, **kw)       # no slice
    assert none["n_levels"][0] == 0 and np.isnan(none["top"][0]) and np.isnan(none["nominal_height"][0])
    one = _levels_agree(*_table([0, 0, 5.0] + [0] * 9), 1.0, 0.5, ground=0.25, **kw)     # one slice: its own body
    assert one["n_levels"][0] == 0 and one["top"][0] == 1.0 + 3 * 0.5 and one["tower_height"][0] == 2.25
    first = _levels_agree(*_table([9.0] + body[1:]), 1.0, 0.5, ground=1.0, **kw)         # an arm at the first slice
    assert first["n_levels"][0] == 1 and first["z_low"][0, 0] == 1.0 and first["z_high"][0, 0] == 1.5
    assert first["nominal_height"][0] == 0.0 and first["rows"][0, 0] == 10.0 and first["width"][0, 0] == 9.0
    last = _levels_agree(*_table(body[:-1] + [9.0]), 1.0, 0.5, **kw)                     # an arm at the last slice
    assert last["n_levels"][0] == 1 and last["z_low"][0, 0] == 1.0 + 11 * 0.5 and last["top"][0] == 7.0
    assert "tower_height" not in last
    two = _levels_agree(*_table([3.0, 9.0, 3.0, 9.5, 9.5, 3.0] + body[6:]), 0.0, 0.5, **kw)   # two arms one slice apart
    assert two["n_levels"][0] == 2 and two["z_low"][0, :2].tolist() == [0.5, 1.5] and two["z_high"][0, :2].tolist() == [1.0, 2.5]
    assert two["rows"][0, :2].tolist() == [10.0, 20.0] and np.isnan(two["z_low"][0, 2:]).all()
    thick = [3.0] * 4 + [9.0] * 8 + [3.0] * 4                                  # eight arm slices > 2G + 1 = 7
    lost = _levels_agree(*_table(thick), 0.0, 0.5, **kw)
    assert lost["n_levels"][0] == 2                                            # its middle is not found: two fragments
    assert lost["z_high"][0, 0] < lost["z_low"][0, 1]
    whole = _levels_agree(*_table([3.0] * 4 + [9.0] * 6 + [3.0] * 6), 0.0, 0.5, **kw)    # 2G = six are found whole
    assert whole["n_levels"][0] == 1 and whole["rows"][0, 0] == 60.0
    seven = _levels_agree(*_table([3.0] * 4 + [9.0] * 7 + [3.0] * 5), 0.0, 0.5, **kw)    # the middle one of 2G + 1 is lost
    assert seven["n_levels"][0] == 2 and seven["rows"][0, :2].tolist() == [30.0, 30.0]
    blind = _levels_agree(*_table([3.0] * 2 + [9.0] * 20 + [3.0] * 2), 0.0, 0.5, **kw)
    assert blind["n_levels"][0] == 2 and (blind["z_high"][0, 0] - blind["z_low"][0, 0]) == 3 * 0.5
    many = [3.0, 9.0] * 10                                                     # ten arms, the lowest max_levels kept
    cut = _levels_agree(*_table(many), 0.0, 0.5, **dict(kw, max_levels=4))
    assert cut["n_levels"][0] == 4 and cut["z_low"].shape == (1, 4) and cut["z_low"][0].tolist() == [0.5, 1.5, 2.5, 3.5]
    _levels_agree(*_table(many), 0.0, 0.5, **dict(kw, max_levels=1))
    # min_rows: a slice of two rows is not occupied, one of three is
    counts = [3] * 12
    counts[5], counts[6] = 2, 3
    edge = _levels_agree(*_table(body[:5] + [9.0, 9.0] + body[7:], counts), 0.0, 0.5, **kw)
    assert edge["n_levels"][0] == 1 and edge["z_low"][0, 0] == 3.0 and edge["rows"][0, 0] == 3.0
    top = _levels_agree(*_table(body[:-1] + [3.0], [3] * 11 + [2]), 0.0, 0.5, **kw)
    assert top["top"][0] == 5.5
    _levels_agree(*_table(body), 0.0, 0.5, **dict(kw, min_rows=11))            # nothing occupied
    # excess exactly at the threshold counts; several towers at once, z0 per tower
    exact = _levels_agree(*_table([3.0, 7.0, 3.0]), 0.0, 0.5, **kw)
    assert exact["n_levels"][0] == 1
    count = np.concatenate([_table(w)[0] for w in (many[:12], body, thick[:12])])
    ext = np.concatenate([_table(w)[1] for w in (many[:12], body, thick[:12])])
    _levels_agree(count, ext, np.array([0.0, 5.0, 12.0]), 0.25, ground=np.array([0.1, 5.2, 11.0]), **dict(kw, arm_window=3.0))
    _levels_agree(count, ext, 2.0, 1.0, **dict(kw, arm_window=0.0))            # G = 0: every slice is its own body


def test_levels_refuse_what_they_cannot_use():
    from pointcloudhookup_amd import ops
    count, ext = _table([3.0] * 4)
    z0 = torch.zeros(1, dtype=torch.float64)
    for kw in (dict(dz=0.0), dict(dz=float("nan")), dict(dz=0.5, arm_window=-1.0), dict(dz=0.5, max_levels=0),
               dict(dz=0.5, arm_excess=float("nan"))):
        with pytest.raises(ValueError):
            ops._tower_levels_of(torch.from_numpy(count), torch.from_numpy(ext), z0, **kw)
    with pytest.raises(TypeError):
        ops.tower_levels(torch.from_numpy(count), torch.from_numpy(ext), 0.0, 0.5)      # CPU tensors: no fallback
    assert "2G + 1" in ops.tower_levels.__doc__


# ------------------------------------------------------------------ the scene
@pytest.mark.parametrize("dz", tp.DZS)
def test_the_scene_has_one_level_per_tower_with_wide_margins(dz):
    for cut in (0.0, 3.5):
        r = tp.scene_reference(dz, cut)                                        # asserts levels and margins
        lv = r["levels"]
        assert np.array_equal(lv["z_low"][:, 0], np.array(sp.LINE_BASES) + 25.0)
        assert np.array_equal(lv["top"], np.array(sp.LINE_BASES) + 30.0)
        assert (np.abs(lv["width"][:, 0] - 16.0) < 0.1).all() and (r["outside"] == 0).all()
        assert r["excess"] >= 2.0 and r["boundary"] >= 1.9e-5
        rows = r["count"].sum(axis=1)
        assert (rows == (2500 if not cut else rows)).all() and (lv["rows"][:, 0] >= 500).all()
    X, perm, offsets, _ = tp.scene_towers()
    tol = tp.ext_tolerance(X, perm, offsets)
    assert (tol > 0).all() and tol.max() < 1e-7                                # far below both margins


def test_the_scene_over_the_terrain_sampled_ground():
    """z0 from the numpy terrain model under the tower axes: the margins are re-asserted for the z0 actually used, and
    the nominal height is 25 m within the slice height and the model's 0.5 m at the tower feet"""
    X, perm, offsets, frames = tp.scene_towers()
    scene = tc.terrain_scene()[0]                                              # terrain_cases.reference's model, alone
    g = tc.scene_grid(scene, tc.CELL)
    _, ground, _ = tc.ground_reference(tc.low_reference(scene, g)[0], tc.WINDOW_CELLS, tc.DH, tc.MAX_GAP)
    z0 = tc.ground_at(g, ground, frames[:, 0], frames[:, 1])
    base = np.array(sp.LINE_BASES)
    assert np.abs(z0 - base).max() <= 0.5
    for dz in tp.DZS:
        f5 = tp.frames5_of(frames, z0)
        B = int(np.ceil(64.0 / dz))
        slot = np.arange(3, dtype=np.int32)
        count, ext, outside = tp.slices_by_sort(X, perm, offsets, f5, slot, 3, dz, B)
        lv = tp.levels_reference(count, ext, z0, dz, ground=z0)
        excess, boundary = tp.margins(X, perm, offsets, f5, slot, 3, dz, B)
        tol = float(tp.ext_tolerance(X, perm, offsets).max())
        # the 2 m of the scene at z0 = base do not carry over (a slice that the arm's edge cuts holds few rows and is
        # narrower); what exactness needs is a margin beyond what another order of the frames' sums can move: a width by
        # 2 tol, a height above z0 by tol times (1 + twice the model's slope), which is below 2 tol here
        assert excess > 10.0 * 2.0 * tol and boundary > 10.0 * 2.0 * tol, (dz, excess, boundary)
        assert (lv["n_levels"] == 1).all() and np.abs(lv["nominal_height"] - 25.0).max() <= dz + 0.5
        assert np.abs(lv["tower_height"] - 30.0).max() <= dz + 0.5


# ------------------------------------------------------------------ the knob
def test_knob_parser():
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.tower_profile_from_env(None) is None and te.tower_profile_from_env("  ") is None
    assert te.tower_profile_from_env("0.5") == dict(dz=0.5, height=64.0, arm_window=3.0, arm_excess=4.0)
    assert te.tower_profile_from_env(" 0.25 , 60 ") == dict(dz=0.25, height=60.0, arm_window=3.0, arm_excess=4.0)
    assert te.tower_profile_from_env("1,100,2,5.5") == dict(dz=1.0, height=100.0, arm_window=2.0, arm_excess=5.5)
    for bad in ("x", "0", "-1", "nan", "inf", "0.5,0", "0.5,nan", "0.5,64,3", "0.5,64,3,4,5", "0.5,64,-1,4",
                "0.5,64,3,nan", "0.5,64,inf,4", "0.25,64.5", "0.1,64", ","):
        with pytest.raises(ValueError):
            te.tower_profile_from_env(bad)
    with pytest.raises(ValueError, match="256"):
        te.tower_profile_from_env("0.25,65")
    assert te.TOWER_PROFILE_COLUMNS == ("ID", "x", "y", "ground_z", "ground_from", "tower_height", "nominal_height",
                                        "lowest_wire", "n_levels", "levels")
    assert te.TOWER_PROFILE_MAX_SLICES == 256


def test_a_malformed_knob_fails_at_import():
    """the knob is read once at import: a fresh interpreter, where the import must fail with a clear ValueError"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PCH_")}
    code = "import pointcloudhookup_amd.utils.tower_extraction as te; print(te.TOWER_PROFILE)"
    run = lambda **kw: subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(env, **kw), capture_output=True,
                                      text=True)
    for value in ("0.5,64,3", "0.1,64", "zero"):
        bad = run(PCH_TOWER_PROFILE=value)
        assert bad.returncode != 0 and "ValueError" in bad.stderr, (value, bad.stderr)
    assert "PCH_TOWER_PROFILE" in run(PCH_TOWER_PROFILE="0.5,64,3").stderr
    good = run(PCH_TOWER_PROFILE="0.5")                                        # it needs no other knob
    assert good.returncode == 0 and "'dz': 0.5" in good.stdout and "'height': 64.0" in good.stdout, good.stderr
    off = run()
    assert off.returncode == 0 and off.stdout.strip() == "None", off.stderr
    empty = run(PCH_TOWER_PROFILE="")
    assert empty.returncode == 0 and empty.stdout.strip() == "None", empty.stderr


def test_csv_rows_and_the_log_line():
    from pointcloudhookup_amd.utils import tower_extraction as te
    nan = float("nan")
    table = dict(ground=torch.tensor([1.0, 2.0]), ground_from=["terrain", "cluster"], top=torch.tensor([31.0, nan]),
                 tower_height=torch.tensor([30.0, nan]), nominal_height=torch.tensor([25.5, nan]),
                 n_levels=torch.tensor([2, 0]), z_low=torch.tensor([[26.5, 29.0], [nan, nan]], dtype=torch.float64),
                 z_high=torch.tensor([[28.0, 29.5], [nan, nan]], dtype=torch.float64),
                 width=torch.tensor([[16.0, 9.25], [nan, nan]], dtype=torch.float64),
                 rows=torch.tensor([[500.0, 40.0], [nan, nan]]), lowest_wire=torch.tensor([20.125, nan]))
    profile = dict(which=torch.tensor([3, 7]), frames5=torch.tensor([[1.0, 2.0, 1.0, 1.0, 0.0], [5.0, 6.0, 2.0, 0.0, 1.0]],
                                                                    dtype=torch.float64), table=table)
    rows = te.tower_profile_rows(profile, ["tower_7", "tower_3"], np.array([100.0, 200.0, 10.0]))
    assert [r[0] for r in rows] == ["tower_7", "tower_3"]                      # towers_info's order
    assert rows[1] == ["tower_3", 101.0, 202.0, 11.0, "terrain", 30.0, 25.5, 20.125, 2, "36.5:38.0:16.0;39.0:39.5:9.25"]
    assert rows[0][:5] == ["tower_7", 105.0, 206.0, 12.0, "cluster"] and rows[0][8:] == [0, ""]
    line = te.tower_profile_line(rows, te.tower_profile_from_env("0.5"))
    assert "杆塔剖面" in line and "杆塔 2" in line and "有横担 1" in line and "地形地面 1" in line and "25.5" in line
