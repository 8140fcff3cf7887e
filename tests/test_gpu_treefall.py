"""Tree fall on the device (pch_treefall_f32, ops.treefall, pipeline.danger_trees, the drop-in's PCH_TREEFALL): every
output must equal the numpy statement of the rule (treefall_cases) bit for bit, one NaN being as good as another -
through ``ops`` and once through the raw C ABI -, whatever the sweep culls."""
import csv

import numpy as np
import pytest
import torch

import clearance_cases as cc
import las_bytes
import shape_cases as sc
import span_cases as sp
import terrain_cases as tc
import treefall_cases as tf
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

TILE = ops.TREEFALL_TILE
RULE = (2.0, 30.0, 0.5, 3.0)                     # h_min, h_max, grow, limit


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(cuda)


def _ground(seed, nx=48, ny=40, cell=2.0, holes=0.06):
    """(grid, ground float32 [ny,nx]): a random sloped grid with some NaN cells"""
    rng = np.random.default_rng(seed)
    g = tc.grid(x0=-10.0, y0=5.0, cell=cell, nx=nx, ny=ny)
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    ground = (0.1 * xx + 0.06 * yy + rng.normal(0.0, 0.3, (ny, nx))).astype(np.float32)
    ground[rng.uniform(size=ground.shape) < holes] = np.nan
    return g, ground


def _spans(K, S, g, seed, half=(5.0, 30.0), up=(8.0, 25.0)):
    """(curves float64 [K,10], segs float64 [K,S,5]): K sagging wires over the grid, ``up`` metres above its slope"""
    rng = np.random.default_rng(seed)
    w, h = g["nx"] * g["cell"], g["ny"] * g["cell"]
    rows = []
    for _ in range(K):
        cx, cy = g["x0"] + rng.uniform(0.0, 1.0) * w, g["y0"] + rng.uniform(0.0, 1.0) * h
        ang = rng.uniform(0.0, 2.0 * np.pi)
        slope = 0.05 * (cx - g["x0"]) + 0.03 * (cy - g["y0"])
        rows.append(cc.curve(cx=cx, cy=cy, cz=slope + rng.uniform(*up), ux=np.cos(ang), uy=np.sin(ang),
                             b=rng.uniform(-0.05, 0.05), c=rng.uniform(0.0, 0.002), m0=-rng.uniform(*half),
                             m1=rng.uniform(*half)))
    curves = np.stack(rows) if K else np.zeros((0, 10))
    return curves, cc.segments_reference(curves, S)[0]


def _rows(n, g, seed, spread=1.1):
    """n float32 rows over the grid (some outside it), 1 m below to 35 m above its slope"""
    rng = np.random.default_rng(seed)
    w, h = g["nx"] * g["cell"], g["ny"] * g["cell"]
    lo = 0.5 * (1.0 - spread)
    x, y = rng.uniform(lo, 1.0 - lo, n) * w, rng.uniform(lo, 1.0 - lo, n) * h
    return np.stack([g["x0"] + x, g["y0"] + y, 0.05 * x + 0.03 * y + rng.uniform(-1.0, 35.0, n)],
                    axis=1).astype(np.float32)


def _run(X, g, ground, curves, segs, rule, cuda, sub=None, skip=None):
    out = ops.treefall(_dev(X, cuda), _dev(curves, cuda), _dev(segs, cuda), g, _dev(ground, cuda), *rule, sub=sub,
                       skip=None if skip is None else _dev(skip, cuda), want_stats=True)
    return {key: v.cpu().numpy() for key, v in out.items()}


def _check(X, g, ground, curves, segs, rule, cuda, what, sub=None, skip=None):
    want = tf.treefall_reference(X, g, ground, curves, segs, *rule, sub=sub, skip=skip)
    got = _run(X, g, ground, curves, segs, rule, cuda, sub=sub, skip=skip)
    for key in tf.OUTPUTS:
        if not tc.same(got[key], want[key]):
            bad = np.flatnonzero(~((got[key] == want[key]) | (np.isnan(got[key].astype(np.float64))
                                                              & np.isnan(want[key].astype(np.float64)))))
            raise AssertionError((what, key, got[key].dtype, len(bad), bad[:5], got[key][bad[:5]], want[key][bad[:5]]))
    assert got["stats"].dtype == np.int64 and got["stats"][:2].tolist() == want["stats"].tolist(), what
    tiles = -(-len(X) // TILE)
    assert 0 <= got["stats"][3] <= tiles * len(curves) and got["stats"][2] >= (want["span"] >= 0).sum(), what
    height = ops.terrain_height(_dev(X, cuda), g, _dev(ground, cuda), sub=sub).cpu().numpy()
    assert tc.same(got["height"], height), what
    return got, want


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4 * TILE + 1])
def test_row_counts_around_the_wave_and_the_tile(cuda, n):
    g, ground = _ground(seed=1)
    curves, segs = _spans(7, 32, g, seed=2)
    got, want = _check(_rows(n, g, seed=100 + n), g, ground, curves, segs, RULE, cuda, n)
    if n >= TILE:
        assert (want["hazard"] == tf.NEAR).any() and (want["hazard"] == tf.STRIKE).any() and want["stats"][1] > 0


@pytest.mark.parametrize("K", [0, 1, 64, 65, 200])
def test_span_counts_around_the_bitmap_word(cuda, K):
    g, ground = _ground(seed=3)
    curves, segs = _spans(K, 4, g, seed=4)
    got, want = _check(_rows(TILE + 1, g, seed=5), g, ground, curves, segs, RULE, cuda, K)
    assert K < 64 or (want["count"] > 0).sum() > 16
    assert K <= 64 or (want["count"][64:] > 0).any()                          # the bitmap's second word owns rows too


@pytest.mark.parametrize("S", [1, 32, 128])
def test_segment_counts(cuda, S):
    g, ground = _ground(seed=6, nx=64, ny=64, cell=1.5)
    curves, segs = _spans(3, S, g, seed=7)
    _check(_rows(TILE + 1, g, seed=8), g, ground, curves, segs, RULE, cuda, S)


def test_no_rows_and_no_spans_at_once(cuda):
    g, ground = _ground(seed=9)
    got, _ = _check(np.zeros((0, 3), np.float32), g, ground, np.zeros((0, 10)), np.zeros((0, 3, 5)), RULE, cuda, "none")
    assert got["stats"].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------ the radius is the row's own
def test_per_row_radius_inside_one_tile(cuda):
    g, ground, curves, segs = tf.level_case()
    X = np.array([[0.0, 20.0, 20.0],          # tall and far: d2 = 400 + 64 = 464 <= R2 = 23^2: accepted (near)
                  [0.0, 6.0, 5.0]],           # short and nearer: d2 = 100 > R2 = 8^2: rejected
                 dtype=np.float32)
    got, _ = _check(X, g, ground, curves[:1], segs[:1], (2.0, 30.0, 0.0, 3.0), cuda, "two rows")
    assert got["span"].tolist() == [0, -1] and got["hazard"].tolist() == [tf.NEAR, tf.CLEAR] and got["dist2"][0] == 464.0
    # the same two among a tile of rows that take no part
    fill = np.tile(np.array([[0.0, 6.0, 1.0]], dtype=np.float32), (TILE - 2, 1))
    got, _ = _check(np.vstack([fill[:500], X, fill[500:]]), g, ground, curves[:1], segs[:1], (2.0, 30.0, 0.0, 3.0),
                    cuda, "tile")
    assert got["span"][500:502].tolist() == [0, -1] and got["count"].tolist() == [1]


def test_nearest_in_plan_and_by_its_own_position_but_another_span_within_reach(cuda):
    """span a hangs right over the row, 30 m up: it is the nearer one in plan, and the nearer one to the row's own
    position 16 m up - but from the foot it is 30 m away, outside R = 16, while span b, 14 m aside and 2 m up, is
    within it"""
    g, ground, _, _ = tf.level_case()
    curves = np.stack([cc.curve(cz=30.0, m0=-32.0, m1=32.0), cc.curve(cy=14.0, cz=2.0, m0=-32.0, m1=32.0)])
    segs, _ = cc.segments_reference(curves, 4)
    X = np.array([[0.0, 0.0, 16.0]], dtype=np.float32)
    top = cc.span_distances(X, curves, segs)[:, 0]
    assert top[0] < top[1]                                                     # the row itself is nearer to a
    got, _ = _check(X, g, ground, curves, segs, (2.0, 30.0, 0.0, 0.0), cuda, "a and b")
    assert got["span"].tolist() == [1] and got["dist2"][0] == 200.0 and got["hazard"].tolist() == [tf.STRIKE]
    assert got["count"].tolist() == [0, 1]


# ------------------------------------------------------------------ feet, not rows
def test_the_wire_below_the_foot_and_a_crown_near_a_wire_its_foot_is_far_from(cuda):
    g, _, _, _ = tf.level_case()
    rule = (2.0, 20.0, 0.0, 3.0)                                               # Rmax = 23
    high = np.full((16, 16), 30.0, dtype=np.float32)
    curves = np.stack([cc.curve(cy=10.0, cz=20.0, m0=-32.0, m1=32.0)])
    segs, _ = cc.segments_reference(curves, 4)
    X = np.array([[0.0, 0.0, 50.0]], dtype=np.float32)                         # H = 20; Z - cz - zhi = 30 > Rmax
    got, _ = _check(X, g, high, curves, segs, rule, cuda, "wire below the foot")
    assert got["span"].tolist() == [0] and got["dist2"][0] == 200.0 and got["hazard"].tolist() == [tf.STRIKE]
    flat = np.zeros((16, 16), dtype=np.float32)
    curves = np.stack([cc.curve(cz=30.0, m0=-32.0, m1=32.0)])
    segs, _ = cc.segments_reference(curves, 4)
    X = np.array([[0.0, 0.0, 20.0]], dtype=np.float32)                         # Z is 10 m from the wire, the foot 30
    got, _ = _check(X, g, flat, curves, segs, rule, cuda, "crown near, foot far")
    assert got["span"].tolist() == [-1] and got["hazard"].tolist() == [tf.CLEAR] and got["stats"][0] == 1


# ------------------------------------------------------------------ boundaries
def test_equalities_of_the_rule(cuda):
    g, ground, curves, segs = tf.level_case()
    X, skip = tf.boundary_rows()
    got, _ = _check(X, g, ground, curves, segs, (2.0, 12.0, 0.0, 3.0), cuda, "boundaries", skip=skip)
    assert tuple(got["hazard"].tolist()) == tf.BOUNDARY_HAZARD and tuple(got["span"].tolist()) == tf.BOUNDARY_SPAN
    assert got["stats"][:2].tolist() == [7, 1]
    zero, _ = _check(X, g, ground, curves, segs, (2.0, 12.0, 0.0, 0.0), cuda, "limit 0", skip=skip)
    assert set(zero["hazard"].tolist()) == {tf.CLEAR, tf.STRIKE}               # class 1 can only be empty
    grown, _ = _check(X, g, ground, curves, segs, (2.0, 12.0, 3.0, 0.0), cuda, "grow 3", skip=skip)
    assert grown["hazard"][[0, 1, 2, 3]].tolist() == [2, 2, 2, 0]
    _check(X, g, ground, curves, segs, (0.0, 0.0, 0.0, 0.0), cuda, "all zero", skip=skip)
    _check(X, g, ground, curves, segs, (2.0, 12.0, 0.0, 3.0), cuda, "bool skip", skip=skip.astype(bool))
    sub = np.array([512.0, -256.0, 64.0], dtype=np.float32)
    _check((X + sub).astype(np.float32), g, ground, curves, segs, (2.0, 12.0, 0.0, 3.0), cuda, "sub", sub=sub, skip=skip)


def test_limit_zero_and_growth_on_random_rows(cuda):
    g, ground = _ground(seed=11)
    curves, segs = _spans(9, 16, g, seed=12)
    X = _rows(2 * TILE + 5, g, seed=13)
    zero, want = _check(X, g, ground, curves, segs, (2.0, 30.0, 0.0, 0.0), cuda, "limit 0")
    assert not (zero["hazard"] == tf.NEAR).any() and (zero["hazard"] == tf.STRIKE).sum() > 10
    grown, _ = _check(X, g, ground, curves, segs, (2.0, 30.0, 4.0, 0.0), cuda, "grow 4")
    assert (grown["hazard"] == tf.STRIKE).sum() > (zero["hazard"] == tf.STRIKE).sum()


def test_two_spans_tied_go_to_the_lower_index(cuda):
    g, ground = _ground(seed=14, holes=0.0)
    curves, segs = _spans(3, 8, g, seed=15)
    curves, segs = curves[[0, 1, 0, 2, 1]], segs[[0, 1, 0, 2, 1]]               # spans 2 and 4 repeat 0 and 1
    got, _ = _check(_rows(TILE + 9, g, seed=16), g, ground, curves, segs, RULE, cuda, "ties")
    assert got["count"][0] > 0 and got["count"][1] > 0 and got["count"][2] == 0 and got["count"][4] == 0


# ------------------------------------------------------------------ culling
def test_a_direction_that_is_not_unit_is_never_culled(cuda):
    g, ground = _ground(seed=17)
    curves, segs = _spans(4, 8, g, seed=18)
    curves[1, 3:5] *= 2.0
    curves[2, 3:5] *= 1.0 + 1e-5
    curves[3, 3:5] = 0.0
    X = _rows(3 * TILE, g, seed=19)
    got, _ = _check(X[np.argsort(X[:, 0])], g, ground, curves, segs, RULE, cuda, "directions")
    assert got["stats"][3] >= 3 * 3                                            # every tile walks the three of them


def test_spans_far_from_every_tile_and_the_cull_is_alive(cuda):
    g, ground = _ground(seed=20, nx=64, ny=64, cell=2.0, holes=0.02)
    curves, segs = _spans(60, 8, g, seed=21, half=(3.0, 6.0), up=(3.0, 7.0))
    far, fsegs = _spans(4, 8, tc.grid(x0=5000.0, y0=-7000.0, cell=2.0, nx=8, ny=8), seed=22)
    curves, segs = np.vstack([far[:2], curves, far[2:]]), np.vstack([fsegs[:2], segs, fsegs[2:]])
    tiles = 32
    X = _rows(tiles * TILE, g, seed=23, spread=1.0)
    X = X[np.lexsort((X[:, 1] // 16.0, X[:, 0] // 32.0))]                      # tiles that keep to a patch of the grid
    got, want = _check(X, g, ground, curves, segs, (2.0, 8.0, 0.0, 1.0), cuda, "spread out")
    assert want["count"][[0, 1, 62, 63]].sum() == 0 and (want["count"] > 0).sum() > 20
    print(f"cull: {got['stats'][3]} of {tiles * len(curves)} (tile, span) pairs walked, {got['stats'][2]} segment loops")
    assert 0 < got["stats"][3] < tiles * len(curves)


def test_a_tile_without_a_row_that_takes_part_and_rows_without_ground(cuda):
    g, ground = _ground(seed=24)
    curves, segs = _spans(5, 8, g, seed=25)
    X = _rows(3 * TILE, g, seed=26)
    skip = np.zeros(len(X), dtype=np.uint8)
    skip[:TILE] = 1                                                            # the first tile is skipped,
    X[TILE:2 * TILE, 2] = X[TILE:2 * TILE, 2] * np.float32(0.0) - np.float32(5.0)       # the second is under the ground
    got, want = _check(X, g, ground, curves, segs, RULE, cuda, "empty tiles", skip=skip)
    assert (got["span"][:2 * TILE] == -1).all() and (got["span"][2 * TILE:] >= 0).any()
    X[5, 0] = np.inf
    X[TILE + 7, 2] = np.nan
    X[2 * TILE + 9, 1] = -np.inf
    _check(X, g, ground, curves, segs, RULE, cuda, "rows that are not finite", skip=skip)
    # no ground anywhere: every finite row that is not skipped is uncovered, nothing is walked
    got, want = _check(X, g, np.full_like(ground, np.nan), curves, segs, RULE, cuda, "uncovered", skip=skip)
    assert got["stats"][0] == 0 and got["stats"][1] == 2 * TILE - 2 and got["stats"][3] == 0
    assert np.isnan(got["height"]).all() and (got["hazard"] == 0).all()
    # a span that takes no part, and all of them
    curves[2, 7] = np.nan
    _check(X, g, ground, curves, segs, RULE, cuda, "NaN span", skip=skip)
    segs[:, 3, 4] = np.inf
    got, _ = _check(X, g, ground, curves, segs, RULE, cuda, "no span takes part", skip=skip)
    assert (got["span"] == -1).all()


def test_the_same_call_twice_and_shuffled_rows(cuda):
    g, ground = _ground(seed=27)
    curves, segs = _spans(12, 32, g, seed=28)
    X = _rows(5 * TILE + 3, g, seed=29)
    a, _ = _check(X, g, ground, curves, segs, RULE, cuda, "first")
    b = _run(X, g, ground, curves, segs, RULE, cuda)
    for key in tf.OUTPUTS + ("stats",):
        assert tc.same(a[key], b[key]), key
    perm = np.random.default_rng(30).permutation(len(X))
    c, _ = _check(X[perm], g, ground, curves, segs, RULE, cuda, "shuffled")
    assert tc.same(c["dist2"], a["dist2"][perm]) and np.array_equal(c["count"], a["count"])


# ------------------------------------------------------------------ refusals and the raw C ABI
def test_refusals(cuda):
    g, ground = _ground(seed=31)
    curves, segs = _spans(2, 4, g, seed=32)
    X = _rows(10, g, seed=33)
    dX, dC, dS, dG = _dev(X, cuda), _dev(curves, cuda), _dev(segs, cuda), _dev(ground, cuda)
    for rule in ((-1.0, 30.0, 0.0, 3.0), (5.0, 4.0, 0.0, 3.0), (2.0, 30.0, -1.0, 3.0), (2.0, 30.0, 0.0, -3.0),
                 (float("nan"), 30.0, 0.0, 3.0), (2.0, float("inf"), 0.0, 3.0)):
        with pytest.raises(ValueError):
            ops.treefall(dX, dC, dS, g, dG, *rule)
    with pytest.raises(ValueError):
        ops.treefall(dX, dC[:, :4], dS, g, dG, *RULE)
    with pytest.raises(ValueError):
        ops.treefall(dX, dC, dS[:1], g, dG, *RULE)
    with pytest.raises(ValueError):
        ops.treefall(dX, dC, torch.zeros((2, 129, 5), dtype=torch.float64, device=cuda), g, dG, *RULE)
    with pytest.raises(ValueError):
        ops.treefall(dX, dC, dS, g, dG[:-1], *RULE)
    with pytest.raises(ValueError):
        ops.treefall(dX, dC, dS, dict(g, cell=0.0), dG, *RULE)
    with pytest.raises(ValueError):
        ops.treefall(dX, dC, dS, g, dG, *RULE, skip=torch.zeros(9, dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError):
        ops.treefall(dX, torch.zeros((4097, 5), dtype=torch.float64, device=cuda),
                     torch.zeros((4097, 1, 5), dtype=torch.float64, device=cuda), g, dG, *RULE)
    with pytest.raises(TypeError):
        ops.treefall(dX.cpu(), dC, dS, g, dG, *RULE)
    with pytest.raises(TypeError):
        ops.treefall(dX.double(), dC, dS, g, dG, *RULE)


def test_the_raw_c_abi(cuda):
    import ctypes as C
    L = _lib.lib()
    g, ground = _ground(seed=34)
    curves, segs = _spans(6, 16, g, seed=35)
    X = _rows(2 * TILE + 7, g, seed=36)
    skip = (np.arange(len(X)) % 11 == 0).astype(np.uint8)
    n, K, S = len(X), len(curves), segs.shape[1]
    want = tf.treefall_reference(X, g, ground, curves, segs, *RULE, skip=skip)
    dX, dk, dG = _dev(X, cuda), _dev(skip, cuda), _dev(ground.reshape(-1), cuda)
    dC, dS = _dev(curves[:, :5], cuda), _dev(segs, cuda)
    mk = lambda m, dt: torch.full((m,), 7, dtype=dt, device=cuda)
    out = dict(dist2=mk(n, torch.float64), span=mk(n, torch.int32), height=mk(n, torch.float32),
               hazard=mk(n, torch.uint8), count=mk(K, torch.int64), strikes=mk(K, torch.int64),
               min_dist2=mk(K, torch.float64), min_row=mk(K, torch.int64), max_height=mk(K, torch.float32),
               max_row=mk(K, torch.int64))
    stats = mk(4, torch.int64)
    need = L.pch_treefall_ws_bytes(n, K, S)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    gc = _lib.TerrainGridC(g["x0"], g["y0"], g["cell"], g["nx"], g["ny"])
    gp = lambda s=gc: C.cast(C.pointer(s), C.c_void_p)

    def call(xyz=None, nn=n, grid=None, gr=None, cv=None, kk=K, ss=S, rule=RULE, d2=None, wsp=None, wb=None, sts=None):
        return L.pch_treefall_f32(p(dX) if xyz is None else xyz, p(dk), nn, None, gp() if grid is None else grid,
                                  p(dG) if gr is None else gr, p(dC) if cv is None else cv, p(dS), kk, ss, *rule,
                                  p(out["dist2"]) if d2 is None else d2, p(out["span"]), p(out["height"]),
                                  p(out["hazard"]), p(out["count"]), p(out["strikes"]), p(out["min_dist2"]),
                                  p(out["min_row"]), p(out["max_height"]), p(out["max_row"]),
                                  p(stats) if sts is None else sts, p(ws) if wsp is None else wsp,
                                  need if wb is None else wb, st)

    assert call() == 0
    torch.cuda.synchronize()
    for key in tf.OUTPUTS:
        assert tc.same(out[key].cpu().numpy(), want[key]), key
    assert stats[:2].tolist() == want["stats"].tolist()
    before = {key: v.clone() for key, v in out.items()}
    assert call(sts=0) == 0                                                    # the statistics are optional
    assert call(wb=need - 1) == -2 and b"workspace" in L.pch_last_error()      # PCH_ERR_WORKSPACE
    host = np.zeros(1 << 16, dtype=np.uint8)
    nan, inf = float("nan"), float("inf")
    bad_grid = _lib.TerrainGridC(0.0, 0.0, 0.0, 1, 1)
    for rc in [call(nn=-1), call(nn=2 ** 31), call(kk=-1), call(kk=4097), call(ss=0), call(ss=129), call(xyz=0),
               call(d2=0), call(gr=0), call(cv=0), call(wsp=0), call(grid=0), call(grid=gp(bad_grid)),
               call(wsp=host.ctypes.data), call(gr=host.ctypes.data), call(rule=(-1.0, 30.0, 0.0, 3.0)),
               call(rule=(5.0, 4.0, 0.0, 3.0)), call(rule=(2.0, 30.0, -1.0, 3.0)), call(rule=(2.0, 30.0, 0.0, -1.0)),
               call(rule=(nan, 30.0, 0.0, 3.0)), call(rule=(2.0, inf, 0.0, 3.0)), call(rule=(2.0, 30.0, inf, 3.0)),
               call(rule=(2.0, 30.0, 0.0, nan))]:
        assert rc == -1                                                        # PCH_ERR_ARG
    torch.cuda.synchronize()
    for key, v in out.items():                                                 # a refused call writes nothing
        assert torch.equal(v.view(torch.uint8), before[key].view(torch.uint8)), key
    # no row: the table is empty - without a row pointer to read; no span: every row answered without a span pointer
    assert L.pch_treefall_f32(0, 0, 0, None, gp(), p(dG), p(dC), p(dS), K, S, *RULE, 0, 0, 0, 0, p(out["count"]),
                              p(out["strikes"]), p(out["min_dist2"]), p(out["min_row"]), p(out["max_height"]),
                              p(out["max_row"]), p(stats), p(ws), need, st) == 0
    torch.cuda.synchronize()
    assert (out["count"] == 0).all() and (out["strikes"] == 0).all() and torch.isinf(out["min_dist2"]).all()
    assert (out["min_row"] == -1).all() and torch.isnan(out["max_height"]).all() and (out["max_row"] == -1).all()
    assert stats.tolist() == [0, 0, 0, 0]
    assert L.pch_treefall_f32(p(dX), p(dk), n, None, gp(), p(dG), 0, 0, 0, S, *RULE, p(out["dist2"]), p(out["span"]),
                              p(out["height"]), p(out["hazard"]), 0, 0, 0, 0, 0, 0, p(stats), p(ws), need, st) == 0
    torch.cuda.synchronize()
    assert torch.isinf(out["dist2"]).all() and (out["span"] == -1).all() and (out["hazard"] == 0).all()
    assert tc.same(out["height"].cpu().numpy(), want["height"]) and stats[:2].tolist() == want["stats"].tolist()
    assert stats[2:].tolist() == [0, 0]


# ------------------------------------------------------------------ pipeline level
def test_danger_trees_against_the_reference(cuda):
    r = tf.reference()
    X, _, _ = tf.stem_scene()
    terrain = pipeline.terrain_model(_dev(X, cuda), cell=tc.CELL, window=12.0, dh=tc.DH, max_gap=16.0)
    assert terrain["grid"] == r["grid"]
    points = _dev(r["points"], cuda)                                         # the rows a ground rule would keep
    spans = pipeline.conductor_spans(points, rule=dict(sc.SCENE_RULE), towers=sp.line_towers())
    K, idx, tol = r["spans"]["nclusters"], r["idx"], r["tol"]
    assert np.array_equal(torch.nonzero(spans["accepted"]).reshape(-1).cpu().numpy(), idx)
    out = pipeline.danger_trees(points, spans, terrain, h_min=tf.H_MIN, h_max=tf.H_MAX, grow=tf.GROW, limit=tf.LIMIT,
                                segments=tf.SEGMENTS, towers=sp.line_towers(), cell=tf.CELL)
    want_span = np.where(r["span"] >= 0, idx[np.maximum(r["span"], 0)], -1).astype(np.int32)
    hazard, span = out["hazard"].cpu().numpy(), out["span"].cpu().numpy()
    assert hazard.dtype == np.uint8 and np.array_equal(hazard, r["hazard"]) and np.array_equal(span, want_span)
    h = out["height"].cpu().numpy()
    ftol = tol + 2.0 ** -20                                                    # (and a float32 of up to 32 m)
    assert np.array_equal(np.isnan(h), np.isnan(r["height"]))
    assert float(np.nanmax(np.abs(h.astype(np.float64) - r["height"]))) <= ftol
    near = r["span"] >= 0
    dist = np.sqrt(out["dist2"].cpu().numpy())
    assert np.isinf(dist[~near]).all() and np.abs(dist[near] - np.sqrt(r["dist2"][near])).max() <= tol
    T = {key: v.cpu().numpy() for key, v in out["table"].items()}
    assert tuple(T) == pipeline.TREEFALL_TABLE_KEYS and all(len(v) == K for v in T.values())
    rest = np.setdiff1d(np.arange(K), idx)
    for key in ("count", "strikes", "min_row", "max_row"):
        assert np.array_equal(T[key][idx], r[key]), key
    has = r["count"] > 0
    worst = float(np.abs(T["min_distance"][idx][has] - np.sqrt(r["min_dist2"][has])).max())
    print(f"danger trees: worst difference of a smallest distance {worst:.3e} m, tol {tol:.3e} m; "
          f"count {r['count'].tolist()}, strikes {r['strikes'].tolist()}")
    assert worst <= tol and np.isinf(T["min_distance"][idx][~has]).all()
    assert np.abs(T["max_height"][idx][has].astype(np.float64) - r["max_height"][has]).max() <= ftol
    assert np.isnan(T["max_height"][idx][~has]).all() and np.abs(T["chord_error"][idx] - r["chord"]).max() <= tol
    assert (T["count"][rest] == 0).all() and (T["min_row"][rest] == -1).all() and np.isnan(T["chord_error"][rest]).all()
    assert np.isinf(T["min_distance"][rest]).all() and np.isnan(T["max_height"][rest]).all()
    # the trees: the reference's rows, exactly; the metres within tol
    trees = out["trees"]
    assert [t["row"] for t in trees] == [t["row"] for t in r["trees"]] and len(trees) >= 3
    for got, want in zip(trees, r["trees"]):
        assert tuple(got) == pipeline.TREEFALL_TREE_KEYS
        assert (got["span"], got["hazard"], got["x"], got["y"]) == (int(idx[want["span"]]), want["hazard"], want["x"],
                                                                    want["y"])
        assert abs(got["ground"] - want["ground"]) <= tol and abs(got["height"] - want["height"]) <= ftol
        assert abs(got["distance"] - want["distance"]) <= tol and abs(got["margin"] - want["margin"]) <= tol + ftol
    # no accepted piece: an empty result, nothing raised
    none = pipeline.danger_trees(points, dict(spans, accepted=torch.zeros_like(spans["accepted"])), terrain)
    assert none["trees"] == [] and not none["hazard"].any() and (none["span"] == -1).all()
    assert not none["table"]["count"].any() and torch.isinf(none["dist2"]).all()
    assert torch.equal(none["height"].view(torch.int32), out["height"].view(torch.int32))
    # ops.treefall on the reference's own curves and ground: the statement bit for bit
    got = ops.treefall(points, _dev(r["curves"], cuda), _dev(r["segs"], cuda), r["grid"], _dev(r["ground"], cuda),
                       tf.H_MIN, tf.H_MAX, tf.GROW, tf.LIMIT, skip=_dev(r["skip"], cuda))
    for key in tf.OUTPUTS:
        assert tc.same(got[key].cpu().numpy(), r[key]), key
    with pytest.raises(ValueError):
        pipeline.danger_trees(points[:-1], spans, terrain)
    with pytest.raises(ValueError):
        pipeline.danger_trees(points, spans, terrain, h_min=5.0, h_max=4.0)
    with pytest.raises(TypeError):
        pipeline.danger_trees(points.cpu(), spans, terrain)


# ------------------------------------------------------------------ drop-in
def test_drop_in_knob_writes_the_tree_fall_table(cuda, tmp_path, monkeypatch):
    from pointcloudhookup_amd.utils import tower_extraction as te
    X, _ = cc.tree_scene()
    rng = np.random.default_rng(1)
    sheet = np.concatenate([sp._line_xy(rng.uniform(-15.0, 165.0, 20000), rng.uniform(-30.0, 30.0, 20000)),
                            rng.uniform(0.0, 0.2, (20000, 1))], axis=1).astype(np.float32)
    lifted = X.copy()
    lifted[:, 2] += np.float32(3.5)
    # one stem 10 m beside an outer conductor of the first span, 32 m tall: the wire hangs some 26 m above its foot
    up = np.arange(2.0, 32.0 + 1e-9, 0.25)
    stem = np.concatenate([sp._line_xy(np.full(len(up), 55.0), np.full(len(up), 16.0))
                           + rng.uniform(-0.05, 0.05, (len(up), 2)), up[:, None]], axis=1).astype(np.float32)
    raw = np.vstack([lifted, sheet, stem])
    scales, offsets = np.array([0.001, 0.001, 0.001]), np.array([0.0, 0.0, 0.0])
    path = str(tmp_path / "line.las")
    las_bytes.build(path, np.round(raw.astype(np.float64) / scales).astype(np.int32), scales=scales, offsets=offsets)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(te, "OBB_MODE", "upright")
    monkeypatch.setattr(te, "DROP_LINEAR", te.drop_linear_from_env("2,0.9,0.5,10"))
    monkeypatch.setattr(te, "SPANS", te.spans_from_env("1,5,9,20"))
    monkeypatch.setattr(te, "TERRAIN", te.terrain_from_env("1,12,0.5,7", spans=True))

    def run():
        logs = []
        return te.extract_towers(path, log_callback=logs.append, min_points=20), logs

    files = lambda: sorted(f.name for f in (tmp_path / "output_towers").iterdir())
    assert te.TREEFALL is None
    off, off_logs = run()
    off_files = files()
    table = tmp_path / "output_towers" / "tree_fall_info.csv"
    assert len(off) == 3 and not table.exists() and not any("倒树隐患" in m for m in off_logs)
    monkeypatch.setattr(te, "TREEFALL", te.treefall_from_env("2,3", spans=True, terrain=True))
    on, logs = run()
    extra = [m for m in logs if "倒树隐患" in m]
    assert len(extra) == 1 and "限距 3 m" in extra[0] and "计算失败" not in extra[0], extra
    assert [m for m in logs if "倒树隐患" not in m] == off_logs
    assert files() == sorted(off_files + ["tree_fall_info.csv"])
    assert len(on) == len(off)
    for a, b in zip(on, off):                                                  # the tower dicts are the same
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    with open(table, newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == te.TREEFALL_COLUMNS and 1 <= len(lines) - 1 <= 2    # the stem, in one cell or two
    assert f"隐患树 {len(lines) - 1} 处" in extra[0]
    with open(tmp_path / "output_towers" / "spans_info.csv", newline="", encoding="utf-8") as f:
        span_ids = [v[0] for v in list(csv.reader(f))[1:]]
    col = te.TREEFALL_COLUMNS.index
    xy = sp._line_xy(np.array([55.0]), np.array([16.0]))[0]
    tallest = max(lines[1:], key=lambda v: float(v[col("height")]))
    for v in lines[1:]:
        assert v[col("span")] in span_ids and v[col("ID")].startswith("tree_") and int(v[col("hazard")]) in (1, 2)
        assert abs(float(v[col("x")]) - xy[0]) < 0.1 and abs(float(v[col("y")]) - xy[1]) < 0.1
        assert -0.01 < float(v[col("ground_z")]) < 0.21
        assert abs(float(v[col("margin")]) - (float(v[col("distance")]) - float(v[col("height")]))) < 1e-5
    # the top of the stem: 32 m less the sheet under it, and it strikes - the wire is some 28 m from its foot
    assert 31.75 < float(tallest[col("height")]) < 32.01 and int(tallest[col("hazard")]) == 2
    assert 27.0 < float(tallest[col("distance")]) < 29.5 and float(tallest[col("margin")]) < -2.0
    # with growth the same stem, and a taller bracket leaves nothing
    monkeypatch.setattr(te, "TREEFALL", te.treefall_from_env("40,3,0,45", spans=True, terrain=True))
    _, logs = run()
    assert any("隐患树 0 处" in m for m in logs)
    with open(table, newline="", encoding="utf-8") as f:
        assert len(list(csv.reader(f))) == 1                                   # the header alone
    table.unlink()
    monkeypatch.setattr(te, "TREEFALL", None)
    again, again_logs = run()
    assert again_logs == off_logs and len(again) == 3 and files() == off_files
