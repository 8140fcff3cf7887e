"""Terrain grid on the device (pch_terrain_low_f32, pch_terrain_ground_f32, pch_terrain_height_f32,
pch_terrain_sample_f64, ops.span_ground_profile, pipeline.terrain_model / height_above_ground / span_ground_clearance,
the drop-in's PCH_TERRAIN): every output must equal the numpy statement of the rule (terrain_cases) bit for bit, one NaN
being as good as another."""
import csv
from fractions import Fraction

import numpy as np
import pytest
import torch

import clearance_cases as cc
import las_bytes
import shape_cases as sc
import span_cases as sp
import terrain_cases as tc
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

TILE = ops.TERRAIN_TILE
EPSG = np.array([437000.0, 3139000.0, 80.0])


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(cuda)


def _rows(n, g, seed, spread=1.0):
    """n float32 rows over the grid (spread > 1: some of them outside it on every side)"""
    rng = np.random.default_rng(seed)
    w, h = g["nx"] * g["cell"], g["ny"] * g["cell"]
    lo = 0.5 * (1.0 - spread)
    return np.stack([g["x0"] + rng.uniform(lo, 1.0 - lo, n) * w, g["y0"] + rng.uniform(lo, 1.0 - lo, n) * h,
                     rng.normal(0.0, 5.0, n)], axis=1).astype(np.float32)


def _low(X, g, cuda, sub=None, skip=None, want_stats=False):
    out = ops.terrain_low(_dev(X, cuda), g, sub=sub, skip=None if skip is None else _dev(skip, cuda),
                          want_stats=want_stats)
    return {key: v.cpu().numpy() for key, v in out.items()}


def _check_low(X, g, cuda, what, sub=None, skip=None):
    want_low, want_count = tc.low_reference(X, g, sub=sub, skip=skip)
    got = _low(X, g, cuda, sub=sub, skip=skip, want_stats=True)
    assert got["low"].dtype == np.float32 and got["count"].dtype == np.int32, what
    if not tc.same(got["low"], want_low) or not np.array_equal(got["count"], want_count):
        bad = np.flatnonzero((got["count"] != want_count).reshape(-1))
        raise AssertionError((what, len(bad), bad[:5], got["low"].reshape(-1)[bad[:5]], want_low.reshape(-1)[bad[:5]]))
    assert got["stats"][0] == want_count.sum(), what
    assert (want_count > 0).sum() <= got["stats"][1] <= max(want_count.sum(), 0), what
    return got


# ------------------------------------------------------------------ lowest return
@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4 * TILE + 1])
def test_row_counts_around_the_wave_and_the_tile(cuda, n):
    g = tc.grid(x0=-4.0, y0=2.5, cell=0.5, nx=9, ny=7)
    _check_low(_rows(n, g, seed=n, spread=1.2), g, cuda, n)


@pytest.mark.parametrize("shape", [(1, 1), (1, 37), (37, 1), (3, 3), (257, 130)])
def test_grid_shapes(cuda, shape):
    g = tc.grid(x0=10.0, y0=-20.0, cell=0.75, nx=shape[0], ny=shape[1])
    got = _check_low(_rows(5000, g, seed=shape[0] + shape[1], spread=1.1), g, cuda, shape)
    assert got["low"].shape == (shape[1], shape[0])


def test_all_rows_in_one_cell(cuda):
    g = tc.grid(cell=2.0, nx=3, ny=3)
    for n in (TILE, 70000):                                                  # 70 000: past any 16-bit tally
        rng = np.random.default_rng(n)
        X = np.stack([rng.uniform(2.0, 3.9, n), rng.uniform(2.0, 3.9, n), rng.normal(0, 3, n)], axis=1).astype(np.float32)
        got = _check_low(X, g, cuda, n)
        assert got["count"][1, 1] == n and got["count"].sum() == n and got["low"][1, 1] == X[:, 2].min()
        assert got["stats"][1] == -(-n // TILE)                              # one flush per tile


def test_a_tile_of_distinct_cells_fills_half_the_table(cuda):
    g = tc.grid(cell=1.0, nx=64, ny=17)
    for n in (TILE, TILE + 1):
        c = np.arange(n) % (64 * 17)
        X = np.stack([(c % 64) + 0.5, (c // 64) + 0.5, np.arange(n) * 0.25 - 100.0], axis=1).astype(np.float32)
        got = _check_low(X, g, cuda, n)
        assert got["stats"][1] == n and (got["count"].reshape(-1)[:n] == 1).all()
    # cells that share their low bits, whatever the table's hash makes of them
    c = (np.arange(TILE) * 2048) % (4096 * 4096)
    g = tc.grid(cell=1.0, nx=4096, ny=4096)
    X = np.stack([(c % 4096) + 0.5, (c // 4096) + 0.5, np.ones(TILE)], axis=1).astype(np.float32)
    part, cell, _ = tc.takes_part(X, g)
    got = _low(X, g, cuda, want_stats=True)
    want = np.bincount(cell[part], minlength=4096 * 4096).astype(np.int32)
    assert np.array_equal(got["count"].reshape(-1), want) and got["stats"][1] == (want > 0).sum()
    assert (got["low"].reshape(-1)[want > 0] == 1.0).all() and np.isnan(got["low"].reshape(-1)[want == 0]).all()


def test_rows_alternating_between_two_cells(cuda):
    g = tc.grid(cell=1.0, nx=2, ny=1)
    n = 3 * TILE + 5
    X = np.stack([(np.arange(n) % 2) + 0.5, np.full(n, 0.5), np.cos(np.arange(n))], axis=1).astype(np.float32)
    got = _check_low(X, g, cuda, "alternating")
    assert got["stats"][1] == 2 * 4


def test_zeros_signs_and_denormals(cuda):
    g = tc.grid(cell=1.0, nx=4, ny=1)
    for z in ([0.0, -0.0], [-0.0, 0.0]):
        X = np.array([[0.5, 0.5, z[0]], [0.5, 0.5, z[1]], [1.5, 0.5, 0.0], [2.5, 0.5, -0.0]], dtype=np.float32)
        got = _check_low(X, g, cuda, z)
        assert np.signbit(got["low"][0, 0]) and not np.signbit(got["low"][0, 1]) and np.signbit(got["low"][0, 2])
    z = np.array([1e-45, -1e-45, 3e-39, -3e-39, 1.0, -1.0, 3.4e38, -3.4e38, 1e-45, 2e-45], dtype=np.float32)
    X = np.stack([np.array([0, 0, 1, 1, 2, 2, 3, 3, 1, 1]) + 0.5, np.full(10, 0.5), z], axis=1).astype(np.float32)
    got = _check_low(X, g, cuda, "denormals")
    assert got["low"][0].tolist() == [z[1], z[3], -1.0, z[7]] and got["low"][0, 0] < 0


def test_nonfinite_rows_and_a_tile_without_a_finite_row(cuda):
    g = tc.grid(cell=1.0, nx=5, ny=5)
    X = _rows(3 * TILE, g, seed=5)
    X[TILE:2 * TILE, 2] = np.nan                                             # a tile in which no row takes part
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        for a in range(3):
            X[11 * (3 * k + a) + 2, a] = v
    got = _check_low(X, g, cuda, "nonfinite")
    assert got["count"].sum() == 2 * TILE - 9
    Y = np.full((TILE + 3, 3), np.nan, dtype=np.float32)
    got = _check_low(Y, g, cuda, "all nan")
    assert got["count"].sum() == 0 and np.isnan(got["low"]).all() and got["stats"].tolist() == [0, 0]


def test_rows_outside_on_edges_and_where_the_quotient_rounds_up(cuda):
    g = tc.grid(x0=0.0, y0=0.0, cell=0.1, nx=200, ny=3)
    # every float32 at and next to a multiple of the cell: some lie below k*cell and still divide to k
    k = np.arange(0, 202)
    base = (k * 0.1).astype(np.float32)
    xs = np.concatenate([base, np.nextafter(base, np.float32(-1)), np.nextafter(base, np.float32(1e9))])
    ks = np.concatenate([k, k, k])
    up = [i for i in range(len(xs)) if ks[i] > 0 and Fraction(float(xs[i])) < ks[i] * Fraction(0.1)
          and np.floor(float(xs[i]) / 0.1) == ks[i]]
    assert len(up) > 10                                                      # the case is among them
    X = np.stack([xs, np.full(len(xs), 0.15), np.arange(len(xs), dtype=np.float64)], axis=1).astype(np.float32)
    _check_low(X, g, cuda, "edges in x")
    X = X[:, [1, 0, 2]].copy()
    _check_low(X, tc.grid(x0=0.0, y0=0.0, cell=0.1, nx=3, ny=200), cuda, "edges in y")
    # outside on every side, on the near and on the far edge
    g = tc.grid(x0=-2.0, y0=3.0, cell=0.5, nx=4, ny=6)
    pts = [(-2.0, 3.0), (0.0, 6.0), (-2.0, 6.0), (0.0, 3.0), (-0.0001, 5.9999), (-1.0, 4.0),
           (-2.0001, 4.0), (0.5, 4.0), (-1.0, 2.9999), (-1.0, 6.5), (-1e30, 4.0), (1e30, 4.0), (-1.0, -1e30), (-1.0, 1e30)]
    X = np.array([(x, y, i) for i, (x, y) in enumerate(pts)], dtype=np.float32)
    got = _check_low(X, g, cuda, "outside")
    assert got["count"].sum() == 3 and got["count"][0, 0] == 1 and got["count"][5, 3] == 1


def test_skip_as_uint8_and_as_bool_with_one_tile_skipped(cuda):
    g = tc.grid(cell=1.0, nx=6, ny=4)
    X = _rows(3 * TILE + 9, g, seed=21)
    skip = (np.random.default_rng(22).uniform(0, 1, len(X)) < 0.3).astype(np.uint8)
    skip[TILE:2 * TILE] = 1
    skip[5] = 200                                                            # any non-zero value skips
    a = _check_low(X, g, cuda, "uint8", skip=skip)
    b = ops.terrain_low(_dev(X, cuda), g, skip=_dev(skip != 0, cuda))
    assert tc.same(b["low"].cpu().numpy(), a["low"]) and np.array_equal(b["count"].cpu().numpy(), a["count"])
    none = _check_low(X, g, cuda, "all skipped", skip=np.ones(len(X), np.uint8))
    assert none["count"].sum() == 0


def test_world_coordinates_with_sub3_against_rows_centred_by_torch(cuda):
    g0 = tc.grid(x0=-30.0, y0=-40.0, cell=1.0, nx=64, ny=80)
    raw = (_rows(2 * TILE + 77, g0, seed=31, spread=1.05).astype(np.float64) + EPSG).astype(np.float32)
    sub = EPSG.astype(np.float32)
    g = ops.terrain_grid(_dev(raw, cuda), 1.0, sub=sub)
    assert g == tc.scene_grid(raw, 1.0, sub) and g["nx"] * g["ny"] > 4000
    got = _check_low(raw, g, cuda, "sub3", sub=sub)
    centred = _dev(raw, cuda) - _dev(sub, cuda)
    assert centred.dtype == torch.float32
    b = ops.terrain_low(centred, g)
    assert tc.same(b["low"].cpu().numpy(), got["low"]) and np.array_equal(b["count"].cpu().numpy(), got["count"])
    c = ops.terrain_low(_dev(raw, cuda), g, sub=_dev(sub, cuda))            # sub as a device tensor
    assert tc.same(c["low"].cpu().numpy(), got["low"])
    h, u = ops.terrain_height(_dev(raw, cuda), g, b["low"], sub=sub, want_ground=True)
    wh, wu = tc.height_reference(raw, g, got["low"], sub=sub)
    assert tc.same(h.cpu().numpy(), wh) and tc.same(u.cpu().numpy(), wu)


def test_shuffled_and_sorted_rows_and_the_same_call_twice(cuda):
    g = tc.grid(cell=0.5, nx=120, ny=90)
    X = _rows(20 * TILE, g, seed=41, spread=1.02)
    part, cell, _ = tc.takes_part(X, g)
    order = np.argsort(np.where(part, cell, -1), kind="stable")
    a = _check_low(X, g, cuda, "shuffled")
    b = _check_low(X[order], g, cuda, "sorted")
    assert tc.same(a["low"], b["low"]) and np.array_equal(a["count"], b["count"]) and a["stats"][0] == b["stats"][0]
    print(f"(tile, cell) flushes: shuffled {a['stats'][1]}, sorted by cell {b['stats'][1]}, rows {a['stats'][0]}")
    assert b["stats"][1] < a["stats"][1] <= a["stats"][0]
    again = _low(X, g, cuda, want_stats=True)
    for key in ("low", "count", "stats"):
        assert np.array_equal(again[key].view(np.uint8), a[key].view(np.uint8)), key


def test_refusals(cuda):
    g = tc.grid(cell=1.0, nx=4, ny=4)
    X = _dev(_rows(100, g, seed=51), cuda)
    low = ops.terrain_low(X, g)["low"]
    for bad in (dict(g, cell=0.0), dict(g, cell=np.nan), dict(g, cell=np.inf), dict(g, nx=0), dict(g, ny=-1),
                dict(g, nx=4097, ny=4096)):
        with pytest.raises(ValueError):
            ops.terrain_low(X, bad)
        with pytest.raises(ValueError):
            ops.terrain_sample(torch.zeros((1, 2), dtype=torch.float64, device=cuda), bad, low)
    with pytest.raises(ValueError):
        ops.terrain_low(X, g, skip=torch.zeros(99, dtype=torch.uint8, device=cuda))
    with pytest.raises(ValueError):
        ops.terrain_low(X, g, sub=[1.0, 2.0])
    with pytest.raises(TypeError):
        ops.terrain_low(X.cpu(), g)
    with pytest.raises(TypeError):
        ops.terrain_low(X.double(), g)
    for R, dh, G in ((-1, 0.5, 1), (65, 0.5, 1), (1.5, 0.5, 1), (1, -0.1, 1), (1, np.nan, 1), (1, np.inf, 1),
                     (1, 0.5, -1), (1, 0.5, 257), (True, 0.5, 1)):
        with pytest.raises(ValueError):
            ops.terrain_ground(low, g, R, dh, G)
    with pytest.raises(ValueError):
        ops.terrain_ground(low[:3], g, 1, 0.5, 1)
    with pytest.raises(ValueError):
        ops.terrain_height(X, g, low[:3])
    with pytest.raises(TypeError):
        ops.terrain_height(X, g, low.double())
    with pytest.raises(TypeError):
        ops.terrain_sample(X[:, :2].contiguous(), g, low)                    # float32 positions
    with pytest.raises(ValueError):
        ops.terrain_grid(X, 0.0)
    with pytest.raises(ValueError, match="smallest cell that fits"):
        ops.terrain_grid(_dev(np.array([[0, 0, 0], [5000, 5000, 0]], np.float32), cuda), 1.0)
    with pytest.raises(ValueError, match="64 cells"):
        pipeline.terrain_model(X, window=200.0)
    with pytest.raises(TypeError):
        pipeline.terrain_model(X.cpu())
    assert ops.terrain_grid(torch.zeros((0, 3), dtype=torch.float32, device=cuda), 1.0) == tc.grid()


def test_the_raw_c_abi(cuda):
    import ctypes as C
    L = _lib.lib()
    g = tc.grid(x0=-1.0, y0=-1.0, cell=0.5, nx=11, ny=9)
    X = _rows(TILE + 7, g, seed=61, spread=1.1)
    n, ncells = len(X), 99
    want_low, want_count = tc.low_reference(X, g)
    dX = _dev(X, cuda)
    low = torch.full((ncells,), 7.0, dtype=torch.float32, device=cuda)
    count = torch.full((ncells,), 7, dtype=torch.int32, device=cuda)
    need = L.pch_terrain_low_ws_bytes(n, ncells)
    assert need > 0
    ws = torch.empty(max(need, L.pch_terrain_ground_ws_bytes(ncells)), dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    gc = _lib.TerrainGridC(g["x0"], g["y0"], g["cell"], g["nx"], g["ny"])
    gp = lambda s=gc: C.cast(C.pointer(s), C.c_void_p)

    def call(xyz=None, nn=n, grid=None, out=None, cnt=None, wsp=None, wb=None):
        return L.pch_terrain_low_f32(p(dX) if xyz is None else xyz, 0, nn, None, gp() if grid is None else grid,
                                     p(low) if out is None else out, p(count) if cnt is None else cnt, 0,
                                     p(ws) if wsp is None else wsp, need if wb is None else wb, st)

    assert call() == 0
    torch.cuda.synchronize()
    assert tc.same(low.cpu().numpy(), want_low.reshape(-1)) and np.array_equal(count.cpu().numpy(), want_count.reshape(-1))
    before = (low.clone(), count.clone())
    assert call(wb=need - 1) == -2 and b"workspace" in L.pch_last_error()      # PCH_ERR_WORKSPACE
    host = np.zeros(1 << 16, dtype=np.uint8)
    grids = [_lib.TerrainGridC(0.0, 0.0, c, nx, ny) for c, nx, ny in ((0.0, 1, 1), (-1.0, 1, 1), (float("nan"), 1, 1),
                                                                       (float("inf"), 1, 1), (1.0, 0, 1), (1.0, 1, -1),
                                                                       (1.0, 4097, 4096))]
    for rc in [call(nn=-1), call(nn=2 ** 31), call(xyz=0), call(out=0), call(cnt=0), call(wsp=0), call(grid=0),
               call(wsp=host.ctypes.data)] + [call(grid=gp(b)) for b in grids]:
        assert rc == -1                                                        # PCH_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(low.view(torch.int32), before[0].view(torch.int32)) and torch.equal(count, before[1])
    # no row: every cell NaN with count 0, ground NaN, state 0 - without a pointer to read
    assert L.pch_terrain_low_f32(0, 0, 0, None, gp(), p(low), p(count), 0, p(ws), need, st) == 0
    ground = torch.full((ncells,), 7.0, dtype=torch.float32, device=cuda)
    state = torch.full((ncells,), 7, dtype=torch.uint8, device=cuda)
    gneed = L.pch_terrain_ground_ws_bytes(ncells)

    def gcall(lw=None, R=2, dh=0.5, G=3, grid=None, wsp=None, wb=None, out=None):
        return L.pch_terrain_ground_f32(p(low) if lw is None else lw, gp() if grid is None else grid, R, dh, G, 0,
                                        p(ground) if out is None else out, p(state), p(ws) if wsp is None else wsp,
                                        gneed if wb is None else wb, st)

    assert gcall() == 0
    torch.cuda.synchronize()
    assert torch.isnan(low).all() and (count == 0).all() and torch.isnan(ground).all() and (state == 0).all()
    assert gcall(wb=gneed - 1) == -2
    for rc in (gcall(R=-1), gcall(R=65), gcall(dh=-1.0), gcall(dh=float("nan")), gcall(G=-1), gcall(G=257), gcall(lw=0),
               gcall(out=0), gcall(wsp=0), gcall(lw=host.ctypes.data), gcall(wsp=host.ctypes.data),
               gcall(grid=gp(grids[0]))):
        assert rc == -1
    height = torch.full((n,), 7.0, dtype=torch.float32, device=cuda)
    hcall = lambda xyz=p(dX), nn=n, gr=p(ground), out=p(height), grid=None: L.pch_terrain_height_f32(
        xyz, nn, None, gp() if grid is None else grid, gr, out, 0, st)
    assert hcall() == 0 and hcall(xyz=0, nn=0, out=0) == 0
    for rc in (hcall(nn=-1), hcall(nn=2 ** 31), hcall(xyz=0), hcall(out=0), hcall(gr=0), hcall(gr=host.ctypes.data),
               hcall(xyz=host.ctypes.data), hcall(grid=gp(grids[4]))):
        assert rc == -1
    xy = torch.zeros((5, 2), dtype=torch.float64, device=cuda)
    out = torch.full((5,), 7.0, dtype=torch.float64, device=cuda)
    scall = lambda pos=p(xy), m=5, gr=p(ground), o=p(out): L.pch_terrain_sample_f64(pos, m, gp(), gr, o, st)
    assert scall() == 0 and scall(pos=0, m=0, o=0) == 0
    for rc in (scall(m=-1), scall(m=2 ** 31), scall(pos=0), scall(o=0), scall(gr=0), scall(gr=host.ctypes.data)):
        assert rc == -1
    torch.cuda.synchronize()
    assert torch.isnan(height).all() and torch.isnan(out).all()


# ------------------------------------------------------------------ ground cells and fill
def _check_ground(low, R, dh, G, cuda, what):
    low = np.asarray(low, dtype=np.float32)
    ny, nx = low.shape
    g = tc.grid(cell=1.0, nx=nx, ny=ny)
    want = tc.ground_reference(low, R, dh, G)
    got = ops.terrain_ground(_dev(low, cuda), g, R, dh, G, want_open=True)
    got = [got[key].cpu().numpy() for key in ("open", "ground", "state")]
    for name, a, b in zip(("open", "ground", "state"), got, want):
        assert a.shape == (ny, nx) and tc.same(a, b), (what, name)
    lean = ops.terrain_ground(_dev(low, cuda), g, R, dh, G)                   # the opening kept in the workspace
    assert tc.same(lean["ground"].cpu().numpy(), want[1]) and "open" not in lean
    return dict(open=got[0], ground=got[1], state=got[2])


def _rough(ny, nx, seed, holes=0.15):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    low = (0.05 * xx - 0.03 * yy + rng.normal(0.0, 0.4, (ny, nx))).astype(np.float32)
    low[rng.uniform(0, 1, low.shape) < 0.1] += np.float32(4.0)               # returns that are not ground
    low[rng.uniform(0, 1, low.shape) < holes] = np.nan
    return low


@pytest.mark.parametrize("R", [0, 1, 6, 64])
def test_window_radii(cuda, R):
    out = _check_ground(_rough(70, 150, seed=R), R, 0.5, 4, cuda, R)
    if R == 0:
        assert ((out["state"] & 1) == (out["state"] >> 2)).all()            # every cell that has a row is ground


def test_windows_larger_than_the_grid_and_thin_grids(cuda):
    _check_ground(_rough(9, 13, seed=71), 20, 0.5, 3, cuda, "R > grid")      # clipped at every border and corner
    _check_ground(_rough(1, 300, seed=72), 6, 0.5, 5, cuda, "1 x N")
    _check_ground(_rough(300, 1, seed=73), 6, 0.5, 5, cuda, "N x 1")
    _check_ground(_rough(1, 1, seed=74, holes=0.0), 6, 0.5, 5, cuda, "1 x 1")
    _check_ground(_rough(13, 257, seed=75), 6, 0.3, 256, cuda, "G = 256")


def test_holes_spikes_plateaus_and_an_empty_grid(cuda):
    out = _check_ground(np.full((12, 9), np.nan, np.float32), 2, 0.5, 4, cuda, "all NaN")
    assert (out["state"] == 0).all() and np.isnan(out["ground"]).all() and np.isnan(out["open"]).all()
    low = np.zeros((30, 40), np.float32)
    low[10:20, 15:25] = np.nan                                               # a hole wider than the window's radius
    low[5, 5] = 3.0                                                          # a one-cell spike
    low[22:27, 3:8] = 2.0                                                    # a plateau narrower than the window (5 < 7)
    low[2:10, 28:38] = 2.0                                                   # and one wider (8, 10 > 7)
    out = _check_ground(low, 3, 0.5, 16, cuda, "shapes")
    assert out["state"][5, 5] == 6 and (out["state"][22:27, 3:8] == 6).all() and (out["state"][2:10, 28:38] == 5).all()
    assert (out["state"][10:20, 15:25] == 2).all() and (out["ground"][10:20, 15:25] == 0).all()
    no_ground = np.full((6, 6), np.nan, np.float32)
    no_ground[2, 2], no_ground[2, 3] = 1.0, np.inf                           # an infinite low is above any opening
    out = _check_ground(no_ground, 1, 0.5, 8, cuda, "inf")
    assert out["state"][2, 3] == 6 and out["state"][2, 2] == 5


def test_dh_exactly_at_a_difference_and_the_next_double(cuda):
    low = np.zeros((1, 40), np.float32)
    low[0, 20] = np.float32(0.3)
    d = float(np.float32(0.3))
    at = _check_ground(low, 2, d, 4, cuda, "dh = diff")
    below = _check_ground(low, 2, np.nextafter(d, 0.0), 4, cuda, "dh = the double below")
    assert at["state"][0, 20] == 5 and below["state"][0, 20] == 6 and below["ground"][0, 20] == 0.0


def test_gaps_directions_and_every_state(cuda):
    low = np.full((5, 7), np.nan, dtype=np.float32)
    low[2, 0], low[2, 6], low[0, 3], low[4, 3] = 1.0, 2.0, 4.0, 8.0
    out = _check_ground(low, 0, 0.0, 3, cuda, "four directions")            # (2, 3) finds all four
    assert out["state"][2, 3] == 2 and out["state"][2, 2] == 2 and out["state"][1, 1] == 0
    out = _check_ground(low, 0, 0.0, 2, cuda, "a gap of G + 1 in x")        # only -y and +y are within 2
    assert out["ground"][2, 3] == np.float32((4.0 / 2.0 + 8.0 / 2.0) / (0.5 + 0.5))
    for G in (0, 1):
        out = _check_ground(low, 0, 0.0, G, cuda, G)
        assert (out["state"][np.isnan(low)] == 0).sum() == (31 if G == 0 else 19)     # twelve cells touch a ground cell
    one = np.full((3, 9), np.nan, dtype=np.float32)
    one[1, 0] = 5.0
    out = _check_ground(one, 0, 0.0, 8, cuda, "one direction")
    assert out["ground"][1, 8] == 5.0 and np.isnan(out["ground"][0, 8])
    two = one.copy()
    two[1, 8] = 6.0
    three = two.copy()
    three[0, 4] = 7.0
    for name, a in (("two", two), ("three", three)):
        _check_ground(a, 0, 0.0, 8, cuda, name)
    # bit 0 (ground) needs rows and excludes bit 1 (filled): the states that can occur are 0, 2, 4, 5 and 6
    low = np.zeros((1, 30), dtype=np.float32)
    low[0, 10:14] = 5.0
    low[0, 20], low[0, 27:] = np.nan, np.nan
    out = _check_ground(low, 3, 0.5, 1, cuda, "states")
    assert set(out["state"].reshape(-1).tolist()) == {0, 2, 4, 5, 6}


# ------------------------------------------------------------------ height and sample
def _check_height(X, g, ground, cuda, what, sub=None):
    wh, wu = tc.height_reference(X, g, ground, sub=sub)
    dG = _dev(ground, cuda)
    h, u = ops.terrain_height(_dev(X, cuda), g, dG, sub=sub, want_ground=True)
    h, u = h.cpu().numpy(), u.cpu().numpy()
    assert tc.same(h, wh) and tc.same(u, wu), what
    assert tc.same(ops.terrain_height(_dev(X, cuda), g, dG, sub=sub).cpu().numpy(), wh), what
    # the float64 sample at the float32 rows' own coordinates is the double the height call rounded
    P = tc.frame(X, sub).astype(np.float64)
    s = ops.terrain_sample(_dev(P[:, :2], cuda), g, dG).cpu().numpy()
    assert s.dtype == np.float64 and tc.same(s, tc.ground_at(g, ground, P[:, 0], P[:, 1])), what
    fin = np.isfinite(P).all(axis=1)
    assert tc.same(s[fin].astype(np.float32), u[fin]), what
    with np.errstate(invalid="ignore"):
        assert tc.same(np.where(np.isnan(s[fin]), np.float32(np.nan), (P[fin, 2] - s[fin]).astype(np.float32)), h[fin])
    return h, u


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (9, 1), (2, 2), (40, 23)])
def test_heights_on_centres_borders_and_thin_grids(cuda, shape):
    nx, ny = shape
    g = tc.grid(x0=-3.0, y0=5.0, cell=0.5, nx=nx, ny=ny)
    rng = np.random.default_rng(nx * 50 + ny)
    ground = rng.normal(10.0, 2.0, (ny, nx)).astype(np.float32)
    cx, cy = np.meshgrid(g["x0"] + (np.arange(nx) + 0.5) * 0.5, g["y0"] + (np.arange(ny) + 0.5) * 0.5)
    centres = np.stack([cx.reshape(-1), cy.reshape(-1), np.full(nx * ny, 12.0)], axis=1).astype(np.float32)
    h, u = _check_height(centres, g, ground, cuda, "centres")
    assert np.array_equal(u, ground.reshape(-1))                             # a = b = 0
    n = TILE + 9
    border = _rows(n, g, seed=nx + ny)
    side = rng.integers(0, 4, n)
    edge = rng.uniform(0.0, 0.25, n)                                         # the half-cell border strip: the clamps
    border[side == 0, 0] = (g["x0"] + edge)[side == 0]
    border[side == 1, 0] = (g["x0"] + nx * 0.5 - edge)[side == 1]
    border[side == 2, 1] = (g["y0"] + edge)[side == 2]
    border[side == 3, 1] = (g["y0"] + ny * 0.5 - edge)[side == 3]
    _check_height(border, g, ground, cuda, "border")
    _check_height(_rows(4 * TILE + 1, g, seed=3, spread=1.3), g, ground, cuda, "in and out")
    _check_height(_rows(65, g, seed=4), g, ground, cuda, "sub", sub=np.array([0.25, -0.125, 3.0], np.float32))


def test_heights_over_cells_without_ground_and_for_rows_that_are_not_finite(cuda):
    g = tc.grid(cell=1.0, nx=6, ny=5)
    rng = np.random.default_rng(81)
    ground = rng.normal(0.0, 1.0, (5, 6)).astype(np.float32)
    ground[1, 1] = np.nan                                                    # one NaN corner for the rows around it
    ground[3, 3], ground[3, 4] = np.nan, np.nan                              # two
    ground[0, 4], ground[0, 5], ground[1, 4], ground[1, 5] = (np.nan,) * 4   # four: NaN itself
    X = _rows(2 * TILE, g, seed=82)
    for k, v in enumerate((np.nan, np.inf, -np.inf)):
        for a in range(3):
            X[13 * (3 * k + a) + 1, a] = v
    h, u = _check_height(X, g, ground, cuda, "holes")
    inside, fx, fy = tc.cell_of(g, X[:, 0].astype(np.float64), X[:, 1].astype(np.float64))
    own = np.isnan(ground[fy, fx]) | ~np.isfinite(X).all(axis=1)
    assert np.array_equal(np.isnan(u), own) and np.array_equal(np.isnan(h), own) and 50 < own.sum() < len(X)
    nothing = np.full((5, 6), np.nan, np.float32)
    h, _ = _check_height(X, g, nothing, cuda, "no ground")
    assert np.isnan(h).all()


# ------------------------------------------------------------------ pipeline level
def test_terrain_model_and_heights_against_the_reference(cuda):
    r = tc.reference()
    X, kind = tc.terrain_scene()
    raw = _dev(X, cuda)
    terrain = pipeline.terrain_model(raw, cell=tc.CELL, window=12.0, dh=tc.DH, max_gap=16.0)
    assert pipeline.terrain_cells(tc.CELL, 12.0, 16.0) == (tc.WINDOW_CELLS, tc.MAX_GAP)
    assert terrain["grid"] == r["grid"]
    assert np.array_equal(terrain["state"].cpu().numpy(), r["state"])
    assert np.array_equal(terrain["count"].cpu().numpy(), r["count"])
    ground = terrain["ground"].cpu().numpy()
    assert np.array_equal(np.isnan(ground), np.isnan(r["ground"]))
    has = ~np.isnan(ground)
    tol = r["tol"]
    worst = float(np.abs(ground[has].astype(np.float64) - r["ground"][has]).max())
    print(f"terrain model: worst difference of a ground cell {worst:.3e} m, tol {tol:.3e} m")
    assert worst <= tol and tc.same(terrain["low"].cpu().numpy(), r["low"])
    state = r["state"]
    assert (terrain["n_ground"], terrain["n_filled"], terrain["n_unfilled"]) == (
        int((state & 1).astype(bool).sum()), int((state & 2).astype(bool).sum()), int(((state & 3) == 0).sum()))
    h = pipeline.height_above_ground(raw, terrain).cpu().numpy()
    assert np.array_equal(np.isnan(h), np.isnan(r["height"]))
    assert float(np.abs(h.astype(np.float64) - r["height"]).max()) <= tol + 2.0 ** -20   # (and a float32 of 16 m)
    assert 5.4 < h[kind == 21].min() and h[kind == 20].max() < 0.45
    # skipping the roof's rows leaves the cells under it empty, and they are filled all the same
    bare = pipeline.terrain_model(raw, cell=tc.CELL, window=12.0, dh=tc.DH, max_gap=16.0, skip=_dev(kind == 21, cuda))
    assert bare["n_ground"] == terrain["n_ground"] and (bare["state"] == 6).sum() == 0


def test_span_ground_clearance_against_the_reference(cuda):
    r = tc.reference()
    X, _ = tc.terrain_scene()
    terrain = pipeline.terrain_model(_dev(X, cuda), cell=tc.CELL, window=12.0, dh=tc.DH, max_gap=16.0)
    points = _dev(cc.tree_scene()[0], cuda)                                  # the rows a ground rule would keep
    spans = pipeline.conductor_spans(points, rule=dict(sc.SCENE_RULE), towers=sp.line_towers())
    K, idx, p, tol = r["spans"]["nclusters"], r["idx"], r["profile"], r["tol"]
    out = pipeline.span_ground_clearance(spans, terrain, segments=tc.SEGMENTS, limit=tc.LIMIT)
    assert np.array_equal(out["pieces"].cpu().numpy(), idx)
    T = {key: v.cpu().numpy() for key, v in out["table"].items()}
    assert tuple(T) == pipeline.GROUND_CLEARANCE_TABLE_KEYS and all(len(v) == K for v in T.values())
    rest = np.setdiff1d(np.arange(K), idx)
    assert np.array_equal(T["min_vertex"][idx], p["min_vertex"]) and np.array_equal(T["covered"][idx], p["covered"])
    assert np.array_equal(T["violation"][idx], p["violation"]) and not T["violation"].any()
    worst = float(np.abs(T["min_clearance"][idx] - p["min_clearance"]).max())
    print(f"span ground clearance: worst difference {worst:.3e} m, tol {tol:.3e} m; "
          f"clearances {np.round(T['min_clearance'][idx], 3).tolist()}")
    assert worst <= tol
    assert np.abs(out["clearance"].cpu().numpy() - p["clearance"]).max() <= tol
    assert np.abs(T["min_at"][idx] - p["min_at"]).max() <= tol and np.abs(T["chord_error"][idx] - r["chord"]).max() <= tol
    assert (T["min_vertex"][rest] == -1).all() and np.isinf(T["min_clearance"][rest]).all()
    assert np.isnan(T["chord_error"][rest]).all() and np.isnan(T["min_at"][rest]).all() and (T["covered"][rest] == 0).all()
    # the smallest clearance is the reference's piece; the conductors of one span hang at one height over a
    # cross-slope, so within a span the clearances fall as the ground under their lowest points rises
    assert int(np.argmin(T["min_clearance"][idx])) == int(np.argmin(p["min_clearance"]))
    a = np.radians(sp.LINE_AZIMUTH_DEG)
    station = T["min_at"][idx, 0] * np.cos(a) + T["min_at"][idx, 1] * np.sin(a)
    for trio in (idx[station < sp.LINE_STATIONS[1]], idx[station > sp.LINE_STATIONS[1]]):
        by_ground = np.argsort(T["min_at"][trio, 2])
        assert len(trio) == 3 and (np.diff(T["min_clearance"][trio][by_ground]) < 0).all()
    # one piece breaches at a limit between the smallest clearance and the next one
    breach = pipeline.span_ground_clearance(spans, terrain, segments=tc.SEGMENTS, limit=tc.BREACH_LIMIT)
    v = breach["table"]["violation"].cpu().numpy()
    assert v.sum() == 1 and v[idx[int(np.argmin(p["min_clearance"]))]]
    # no accepted piece: an empty table, nothing raised
    none = pipeline.span_ground_clearance(dict(spans, accepted=torch.zeros_like(spans["accepted"])), terrain)
    assert none["pieces"].numel() == 0 and not none["table"]["violation"].any()
    assert torch.isinf(none["table"]["min_clearance"]).all() and none["clearance"].shape == (0, 33)
    # ops.span_ground_profile on the reference's own curves: the statement bit for bit
    got = ops.span_ground_profile(_dev(r["curves"], cuda), tc.SEGMENTS, r["grid"], _dev(r["ground"], cuda), tc.LIMIT)
    for key in ("clearance", "ground", "covered", "min_clearance", "min_vertex", "min_at", "violation"):
        assert tc.same(got[key].cpu().numpy(), p[key]), key


# ------------------------------------------------------------------ drop-in
def test_drop_in_knob_writes_the_ground_clearance_table(cuda, tmp_path, monkeypatch):
    from pointcloudhookup_amd.utils import tower_extraction as te
    X, _ = cc.tree_scene()
    rng = np.random.default_rng(1)
    sheet = np.concatenate([sp._line_xy(rng.uniform(-15.0, 165.0, 20000), rng.uniform(-30.0, 30.0, 20000)),
                            rng.uniform(0.0, 0.2, (20000, 1))], axis=1).astype(np.float32)
    lifted = X.copy()
    lifted[:, 2] += np.float32(3.5)
    raw = np.vstack([lifted, sheet])
    scales, offsets = np.array([0.001, 0.001, 0.001]), np.array([0.0, 0.0, 0.0])
    path = str(tmp_path / "line.las")
    las_bytes.build(path, np.round(raw.astype(np.float64) / scales).astype(np.int32), scales=scales, offsets=offsets)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(te, "OBB_MODE", "upright")
    monkeypatch.setattr(te, "DROP_LINEAR", te.drop_linear_from_env("2,0.9,0.5,10"))
    monkeypatch.setattr(te, "SPANS", te.spans_from_env("1,5,9,20"))

    def run():
        logs = []
        return te.extract_towers(path, log_callback=logs.append, min_points=20), logs

    files = lambda: sorted(f.name for f in (tmp_path / "output_towers").iterdir())
    assert te.TERRAIN is None
    off, off_logs = run()
    off_files = files()
    table = tmp_path / "output_towers" / "ground_clearance_info.csv"
    assert len(off) == 3 and not table.exists()
    monkeypatch.setattr(te, "TERRAIN", te.terrain_from_env("1,12,0.5,7", spans=True))
    on, logs = run()
    extra = [m for m in logs if "导线对地净空" in m]
    assert len(extra) == 1 and "越限线段 0/6" in extra[0], extra
    assert [m for m in logs if "导线对地净空" not in m] == off_logs
    assert files() == sorted(off_files + ["ground_clearance_info.csv"])
    assert len(on) == len(off)
    for a, b in zip(on, off):                                                  # the tower dicts are the same
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    with open(table, newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == te.TERRAIN_COLUMNS and len(lines) == 1 + 6       # one line per accepted piece
    col = {name: np.array([float(v[i]) for v in lines[1:]]) for i, name in enumerate(te.TERRAIN_COLUMNS) if i}
    with open(tmp_path / "output_towers" / "spans_info.csv", newline="", encoding="utf-8") as f:
        spans = list(csv.reader(f))
    assert [v[0] for v in spans[1:]] == [v[0] for v in lines[1:]]
    z_low = np.array([float(v[te.SPANS_COLUMNS.index("z_low")]) for v in spans[1:]])
    length = np.array([float(v[te.SPANS_COLUMNS.index("length")]) for v in spans[1:]])
    # the sheet lies between 0 and 0.2 m and the wires hang 3.5 m higher than in the scene: the lowest vertex over it
    # is within the sheet's 0.2 m of the curve's lowest point
    assert np.array_equal(col["length"], length) and (col["covered"] == 33).all() and not col["violation"].any()
    assert (col["ground_z"] > -0.01).all() and (col["ground_z"] < 0.21).all()
    assert np.abs(col["z"] - col["ground_z"] - col["min_clearance"]).max() < 1e-9
    assert (col["z"] - z_low > -1e-3).all() and (col["z"] - z_low < 0.25).all()
    assert (col["chord_error"] > 1e-3).all() and (col["chord_error"] < 2e-3).all()
    # a limit above the wires: every piece breaches
    monkeypatch.setattr(te, "TERRAIN", te.terrain_from_env("1,12,0.5,40", spans=True))
    _, logs = run()
    assert any("越限线段 6/6" in m for m in logs)
    table.unlink()
    monkeypatch.setattr(te, "TERRAIN", None)
    again, again_logs = run()
    assert again_logs == off_logs and len(again) == 3 and files() == off_files
