"""Tower profile on the device (pch_cluster_slices_f32, ops.cluster_slices / tower_levels, pipeline.tower_profile, the
drop-in's PCH_TOWER_PROFILE): every output of the slice table must equal the numpy statement of the rule
(tower_profile_cases) bit for bit, through ``ops`` and through the raw C ABI."""
import csv

import numpy as np
import pytest
import torch

import clearance_cases as cc
import las_bytes
import shape_cases as sc
import span_cases as sp
import terrain_cases as tc
import tower_profile_cases as tp
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

BLOCK = ops.SLICES_BLOCK
EPSG = np.array([437000.0, 3139000.0, 80.0])


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(cuda)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(got, want, what):
    """count, ext and outside bit for bit (ext holds no NaN: an empty slice is +-inf)"""
    for name, g, w in zip(("count", "ext", "outside"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        if not np.array_equal(_bits(g), _bits(w)):
            bad = np.argwhere(_bits(g) != _bits(w))
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def _case(n, K, T, seed, extra=0, origin=(0.0, 0.0, 0.0), span=40.0):
    """n grouped float32 rows in K clusters of random sizes (some empty), ``extra`` entries behind offsets[K] that name
    rows far outside everything, frames around the rows and slots over -1..T"""
    rng = np.random.default_rng(seed)
    o = np.asarray(origin, dtype=np.float64)
    rows = o + np.stack([rng.uniform(-8.0, 8.0, n), rng.uniform(-8.0, 8.0, n), rng.uniform(-3.0, span, n)], axis=1)
    wild = o + np.stack([rng.uniform(-500.0, 500.0, extra), rng.uniform(-500.0, 500.0, extra),
                         rng.uniform(0.0, span, extra)], axis=1)
    X = np.concatenate([rows, wild]).astype(np.float32)
    mix = rng.permutation(n + extra)
    X = X[mix]
    where = np.argsort(mix)                                               # where each original row went
    cuts = np.sort(rng.integers(0, n + 1, max(K - 1, 0))) if K else np.zeros(0, np.int64)
    offsets = np.concatenate([[0], cuts, [n]]).astype(np.int64) if K else np.zeros(1, np.int64)
    perm = np.concatenate([where[rng.permutation(n)], where[n:]]).astype(np.int32)
    theta = rng.uniform(0.0, np.pi, K)
    frames5 = np.stack([o[0] + rng.normal(0.0, 1.0, K), o[1] + rng.normal(0.0, 1.0, K), o[2] + rng.uniform(-1.0, 1.0, K),
                        np.cos(theta), np.sin(theta)], axis=1).reshape(K, 5)
    slot = rng.integers(-1, T + 1, K).astype(np.int32)
    if K:
        slot[rng.integers(0, K)] = 0
    return X, perm, offsets, frames5, slot


def _run(X, perm, offsets, frames5, slot, T, dz, B, cuda):
    K = len(offsets) - 1
    out = ops.cluster_slices(_dev(X, cuda), _dev(perm, cuda), _dev(offsets, cuda), K,
                             _dev(np.asarray(frames5, dtype=np.float64).reshape(K, 5), cuda),
                             _dev(np.asarray(slot, dtype=np.int32), cuda), T, dz, B)
    return tuple(out[key].cpu().numpy() for key in ("count", "ext", "outside"))


def _check(X, perm, offsets, frames5, slot, T, dz, B, cuda, what):
    want = tp.slices_reference(X, perm, offsets, frames5, slot, T, dz, B)
    got = _run(X, perm, offsets, frames5, slot, T, dz, B, cuda)
    _same(got, want, what)
    return got


# ------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 17])
def test_grouped_rows_around_the_wave_and_the_block(cuda, n):
    for K, extra in ((1, 0), (3, 0), (3, 9)):                              # n_grouped = n + extra entries of perm
        got = _check(*_case(n, K, 2, seed=100 + n + K, extra=extra), 2, 0.5, 64, cuda, (n, K, extra))
        assert got[0].sum() + got[2].sum() <= n


@pytest.mark.parametrize("K", [0, 1, 3, 65])
def test_cluster_counts_with_empty_clusters_and_noise_entries(cuda, K):
    case = _case(2 * BLOCK + 5, K, 4, seed=7 + K, extra=33)
    got = _check(*case, 4, 0.5, 96, cuda, K)
    # the entries behind offsets[K] name rows 500 m out: had one been read, an extent would show it
    assert np.abs(got[1][np.isfinite(got[1])]).max(initial=0.0) < 40.0
    if K == 0:
        assert (got[0] == 0).all() and (got[2] == 0).all() and np.array_equal(got[1][0, 0], tp.EMPTY)


@pytest.mark.parametrize("B", [1, 2, 255, 256])
def test_slice_counts(cuda, B):
    dz = 40.0 / B if B > 2 else 0.5
    _check(*_case(BLOCK + 77, 3, 2, seed=B), 2, dz, B, cuda, B)


def test_clusters_of_no_row_one_row_and_one_over_four_blocks(cuda):
    X, perm, _, _, _ = _case(4 * BLOCK + 40, 1, 1, seed=3)
    offsets = np.array([0, 0, 1, 1, 30, 30 + 3 * BLOCK + 100, len(perm)], dtype=np.int64)   # 0, 1, 0, 29, 4 blocks, rest
    rng = np.random.default_rng(4)
    K = len(offsets) - 1
    frames5 = np.stack([rng.normal(0, 1, K), rng.normal(0, 1, K), np.full(K, -3.5), np.ones(K), np.zeros(K)], axis=1)
    _check(X, perm, offsets, frames5, np.arange(K, dtype=np.int32), K, 0.5, 128, cuda, "own slots")
    _check(X, perm, offsets, frames5, np.zeros(K, dtype=np.int32), 1, 0.5, 128, cuda, "one slot")


def test_two_hundred_clusters_of_three_rows(cuda):
    X, perm, _, _, _ = _case(600, 1, 1, seed=11, extra=5)
    offsets = (3 * np.arange(201)).astype(np.int64)
    rng = np.random.default_rng(12)
    th = rng.uniform(0, np.pi, 200)
    frames5 = np.stack([rng.normal(0, 1, 200), rng.normal(0, 1, 200), rng.uniform(-4, 0, 200), np.cos(th), np.sin(th)],
                       axis=1)
    got = _check(X, perm, offsets, frames5, np.arange(200, dtype=np.int32), 200, 0.5, 128, cuda, "own slots")
    assert (got[0].sum(axis=1) + got[2].sum(axis=1) == 3).all()
    _check(X, perm, offsets, frames5, (np.arange(200) % 7).astype(np.int32), 7, 0.5, 128, cuda, "seven slots")


# ------------------------------------------------------------------ boundaries
def test_rows_on_slice_boundaries_and_around_the_table(cuda):
    B, dz, z0 = 16, 0.5, np.float32(3.0)
    h = np.concatenate([np.arange(B + 1) * dz, [np.nextafter(np.float32(z0), np.float32(-np.inf)) - z0,
                                                 np.nextafter(np.float32(z0 + B * dz), np.float32(0)) - z0]])
    X = np.stack([np.linspace(-2, 2, len(h)), np.linspace(1, -1, len(h)), z0 + h], axis=1).astype(np.float32)
    perm = np.arange(len(X), dtype=np.int32)
    offsets = np.array([0, len(X)], dtype=np.int64)
    f5 = np.array([[0.0, 0.0, float(z0), 1.0, 0.0]])
    count, ext, outside = _check(X, perm, offsets, f5, [0], 1, dz, B, cuda, "boundaries")
    # h = j dz opens slice j; h = B dz is above; the float32 below z0 is below; the float32 below the top is in B - 1
    assert count[0].tolist() == [1] * (B - 1) + [2] and outside[0].tolist() == [1, 1]


def test_signed_zeros_in_one_slice(cuda):
    X = np.array([[0.0, 0.0, 1.0], [-0.0, -0.0, 1.1], [0.0, -0.0, 1.2]], dtype=np.float32)
    perm, offsets = np.arange(3, dtype=np.int32), np.array([0, 3], dtype=np.int64)
    f5 = np.array([[0.0, 0.0, 1.0, 1.0, 0.0]])
    count, ext, _ = _check(X, perm, offsets, f5, [0], 1, 0.5, 2, cuda, "zeros")
    s, t, _ = tp.row_terms(X, perm, f5[0], 0.5)
    assert np.signbit(s).any() and not np.signbit(s).all() and np.signbit(t).any() and not np.signbit(t).all()
    assert count[0, 0] == 3 and np.signbit(ext[0, 0]).tolist() == [True, False, True, False] and (ext[0, 0] == 0).all()


# ------------------------------------------------------------------ participation
def test_clusters_that_take_no_part_move_no_bit(cuda):
    X, perm, offsets, frames5, _ = _case(2 * BLOCK + 9, 6, 3, seed=21)
    slot = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    base = _check(X, perm, offsets, frames5, slot, 3, 0.5, 96, cuda, "all")
    for k in range(6):
        rest = tp.slices_reference(X, perm, offsets, frames5, np.where(np.arange(6) == k, -1, slot), 3, 0.5, 96)
        for bad_slot in (-1, 3, 2 ** 31 - 1, -2 ** 31):
            _same(_run(X, perm, offsets, frames5, np.where(np.arange(6) == k, bad_slot, slot), 3, 0.5, 96, cuda), rest,
                  (k, bad_slot))
        for c in range(5):
            for v in (np.nan, np.inf, -np.inf):
                f = frames5.copy()
                f[k, c] = v
                _same(_run(X, perm, offsets, f, slot, 3, 0.5, 96, cuda), rest, (k, c, v))
        assert offsets[k + 1] == offsets[k] or not np.array_equal(base[0], rest[0]) or not np.array_equal(base[2], rest[2])


def test_two_clusters_sharing_a_slot_equal_their_union(cuda):
    X, perm, _, _, _ = _case(BLOCK + 200, 1, 1, seed=31)
    f = np.array([0.3, -0.2, -3.0, np.cos(0.4), np.sin(0.4)])
    cut = BLOCK - 100
    two = _check(X, perm, np.array([0, cut, len(perm)], dtype=np.int64), np.stack([f, f]), [0, 0], 1, 0.5, 96, cuda, "two")
    one = _check(X, perm, np.array([0, len(perm)], dtype=np.int64), f[None, :], [0], 1, 0.5, 96, cuda, "one")
    _same(two, one, "union")


# ------------------------------------------------------------------ rows
def test_rows_that_are_not_finite(cuda):
    X, perm, offsets, frames5, _ = _case(BLOCK + 30, 2, 2, seed=41)
    X = X.copy()
    rows = perm[:24].reshape(8, 3)
    for i, v in enumerate((np.nan, np.inf, -np.inf)):
        X[rows[0:2, i], 0] = v                                            # x: s and t are not finite -> not binned
        X[rows[2:4, i], 1] = v
    X[rows[4, 0], 2] = np.nan                                             # z NaN: counted nowhere
    X[rows[5, 0], 2] = np.inf                                             # z +inf: above
    X[rows[6, 0], 2] = -np.inf                                            # z -inf: below
    slot = np.array([0, 1], dtype=np.int32)
    count, ext, outside = _check(X, perm, offsets, frames5, slot, 2, 0.5, 96, cuda, "non-finite")
    clean = tp.slices_reference(np.where(np.isfinite(X), X, 0), perm, offsets, frames5, slot, 2, 0.5, 96)
    assert np.isfinite(ext[count > 0]).all()
    assert count.sum() + outside.sum() < clean[0].sum() + clean[2].sum()
    only = np.zeros_like(X)
    only[:, 2] = [np.inf, -np.inf, np.nan][0]
    c2, e2, o2 = _check(only[:5], np.arange(5, dtype=np.int32), np.array([0, 5], dtype=np.int64),
                        np.array([[0.0, 0.0, 0.0, 1.0, 0.0]]), [0], 1, 0.5, 8, cuda, "inf z")
    assert c2.sum() == 0 and o2.tolist() == [[0, 5]]


def test_epsg_scale_coordinates_and_a_direction_that_is_not_unit(cuda):
    X, perm, offsets, frames5, slot = _case(3 * BLOCK + 1, 5, 3, seed=51, origin=EPSG)
    _check(X, perm, offsets, frames5, slot, 3, 0.25, 200, cuda, "epsg")
    f = frames5.copy()
    f[:, 3:5] *= np.array([2.5, 0.001, 7.0, 1e-9, 1e6])[:, None]
    got = _check(X, perm, offsets, f, slot, 3, 0.25, 200, cuda, "not unit")
    assert np.isfinite(got[1][got[0] > 0]).all()


# ------------------------------------------------------------------ call level
def test_the_same_call_twice_and_refusals_through_ops(cuda):
    case = _case(2 * BLOCK + 3, 4, 3, seed=61, extra=7)
    a = _run(*case, 3, 0.5, 64, cuda)
    b = _run(*case, 3, 0.5, 64, cuda)
    _same(a, b, "twice")
    X, perm, offsets, frames5, slot = (_dev(v, cuda) for v in case)
    call = lambda **kw: ops.cluster_slices(**dict(dict(xyz=X, perm=perm, offsets=offsets, nclusters=4, frames5=frames5,
                                                       slot=slot, ntables=3, dz=0.5, nslices=64), **kw))
    call()
    for bad in (dict(ntables=0), dict(ntables=4097), dict(nslices=0), dict(nslices=257), dict(ntables=4096, nslices=257),
                dict(ntables=4097, nslices=256), dict(ntables=4096 + 1, nslices=1), dict(ntables=4096, nslices=256.5),
                dict(ntables=True), dict(dz=0.0), dict(dz=-1.0), dict(dz=float("nan")), dict(dz=float("inf")),
                dict(nclusters=3), dict(frames5=frames5[:3]), dict(slot=slot[:3])):
        with pytest.raises(ValueError):
            call(**bad)
    # 4096 x 256 entries is the largest table: T * B <= 2^20
    assert ops.SLICES_MAX_TABLES * ops.SLICES_MAX == ops.SLICES_MAX_ENTRIES
    for bad in (dict(xyz=X.cpu()), dict(xyz=X.double()), dict(perm=perm.long()), dict(offsets=offsets.int()),
                dict(frames5=frames5.float()), dict(slot=slot.long())):
        with pytest.raises(TypeError):
            call(**bad)


def test_the_raw_c_abi(cuda):
    L = _lib.lib()
    X, perm, offsets, frames5, slot = _case(BLOCK + 40, 3, 2, seed=71, extra=4)
    n, K, T, B, dz = len(perm), 3, 2, 32, 1.5
    want = tp.slices_reference(X, perm, offsets, frames5, slot, T, dz, B)
    dX, dperm, doff, df, ds = (_dev(v, cuda) for v in (X, perm, offsets, frames5, slot))
    count = torch.full((T, B), 7, dtype=torch.int32, device=cuda)
    ext = torch.full((T, B, 4), 7.0, dtype=torch.float64, device=cuda)
    outside = torch.full((T, 2), 7, dtype=torch.int64, device=cuda)
    need = L.pch_cluster_slices_ws_bytes(n, K, T, B)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    state = lambda: tuple(v.cpu().numpy() for v in (count, ext, outside))

    def call(xyz=None, pm=None, off=None, nn=n, kk=K, fr=None, sl=None, tt=T, step=dz, bb=B, cnt=None, ex=None, out=None,
             wsp=None, wb=None):
        pick = lambda v, d: p(d) if v is None else v
        return L.pch_cluster_slices_f32(pick(xyz, dX), pick(pm, dperm), pick(off, doff), nn, kk, pick(fr, df),
                                        pick(sl, ds), tt, step, bb, pick(cnt, count), pick(ex, ext), pick(out, outside),
                                        pick(wsp, ws), need if wb is None else wb, st)

    assert call() == 0
    torch.cuda.synchronize()
    _same(state(), want, "raw")
    before = state()
    assert call(wb=need - 1) == -2 and b"workspace" in L.pch_last_error()      # PCH_ERR_WORKSPACE
    host = np.zeros(1 << 16, dtype=np.uint8).ctypes.data
    refused = [call(nn=-1), call(nn=2 ** 31), call(kk=-1), call(tt=0), call(tt=4097), call(bb=0), call(bb=257),
               call(step=0.0), call(step=-1.0), call(step=float("nan")), call(step=float("inf")),
               call(xyz=0), call(pm=0), call(off=0), call(fr=0), call(sl=0), call(cnt=0), call(ex=0), call(out=0),
               call(wsp=0), call(xyz=host), call(pm=host), call(off=host), call(fr=host), call(sl=host), call(cnt=host),
               call(ex=host), call(out=host), call(wsp=host)]
    assert refused == [-1] * len(refused)                                      # PCH_ERR_ARG
    torch.cuda.synchronize()
    _same(state(), before, "a refused call writes nothing")
    # T * B beyond 2^20 (the buffers of such a call are never touched: it is refused on its sizes)
    assert call(tt=4097, bb=256) == -1 and L.pch_cluster_slices_ws_bytes(n, K, 4096, 256) > 0
    # no row, or no cluster: the tables are still written, without a pointer to read
    for kw in (dict(xyz=0, pm=0, nn=0), dict(xyz=0, pm=0, off=0, fr=0, sl=0, kk=0), dict(xyz=0, pm=0, off=0, fr=0, sl=0,
                                                                                       nn=0, kk=0)):
        count.fill_(7), ext.fill_(7.0), outside.fill_(7)
        assert call(**kw) == 0
        torch.cuda.synchronize()
        c, e, o = state()
        assert (c == 0).all() and (o == 0).all() and (e == np.array(tp.EMPTY)).all(), kw


# ------------------------------------------------------------------ pipeline level
PIPE = dict(eps=3.0, min_points=20, offset=11.5)          # a threshold of z = 14.0: above the whole ground sheet


def _pipeline_inputs(cuda):
    X, kind = tc.terrain_scene()
    raw = _dev(X, cuda)
    out = pipeline.cluster_points(raw, chunk_size=0, want_index=True, drop_linear=dict(sc.SCENE_RULE), **PIPE)
    centroid = np.asarray(out["ground"]["centroid"], dtype=np.float32)
    terrain = pipeline.terrain_model(raw, sub=centroid, cell=tc.CELL, window=12.0, dh=tc.DH, max_gap=16.0)
    gf = ops.ground_filter(raw, 25.0, PIPE["offset"], 1.0, 1000, want_index=False)
    towers = sp.line_towers() - centroid.astype(np.float64)
    spans = pipeline.conductor_spans(gf["points"], rule=dict(sc.SCENE_RULE), towers=towers)
    K = int(out["nclusters"])
    R = out["ground"]["points"].cpu().numpy()
    src = out["ground"]["index"].cpu().numpy()
    perm, offsets = out["perm"].cpu().numpy(), out["offsets"].cpu().numpy()
    tower_rows = np.array([(kind[src[perm[offsets[k]:offsets[k + 1]]]] == 0).sum() for k in range(K)])
    which = np.flatnonzero(tower_rows > 500)
    return dict(X=X, kind=kind, raw=raw, out=out, centroid=centroid, terrain=terrain, spans=spans, K=K, R=R, perm=perm,
                offsets=offsets, which=which)


def test_tower_profile_against_the_reference(cuda):
    s = _pipeline_inputs(cuda)
    which, R, perm, offsets, K = s["which"], s["R"], s["perm"], s["offsets"], s["K"]
    assert len(which) == 3                                                     # three profiled towers
    dz, B = 0.5, 128
    prof = pipeline.tower_profile(s["out"], which=which, terrain=s["terrain"], spans=s["spans"], dz=dz)
    assert tuple(prof["table"]) == pipeline.TOWER_PROFILE_TABLE_KEYS and prof["count"].shape == (3, B)
    assert np.array_equal(prof["which"].cpu().numpy(), which)
    T = {key: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for key, v in prof["table"].items()}
    assert T["ground_from"] == ["terrain"] * 3
    # the reference: numpy frames (its own order of sums) and the numpy terrain model in stage B's frame
    count, origin, M, _ = sp.moments_reference(R, perm, offsets)
    frames = sp.frames_reference(count, origin, M)
    g = tc.scene_grid(s["X"], tc.CELL, sub=s["centroid"])
    assert g == s["terrain"]["grid"]
    low, _ = tc.low_reference(s["X"], g, sub=s["centroid"])
    _, ground, _ = tc.ground_reference(low, tc.WINDOW_CELLS, tc.DH, tc.MAX_GAP)
    z0 = tc.ground_at(g, ground, frames[:, 0], frames[:, 1])
    assert not np.isnan(z0[which]).any()
    f5 = tp.frames5_of(frames, np.where(np.isnan(z0), 0.0, z0))
    slot = np.full(K, -1, dtype=np.int32)
    slot[which] = np.arange(3)
    want = tp.slices_reference(R, perm, offsets, f5, slot, 3, dz, B)
    # tolerances: the frames' sums are taken in the library's order
    tol = float(tp.ext_tolerance(R, perm, offsets)[which].max())
    G = ground.astype(np.float64)
    with np.errstate(invalid="ignore"):
        slope = max(np.nanmax(np.abs(np.diff(G, axis=0))), np.nanmax(np.abs(np.diff(G, axis=1)))) / tc.CELL
    tol_z0 = tol * (1.0 + 2.0 * float(slope)) + 4.0 * tp.U * float(np.abs(z0[which]).max())
    got_f5 = prof["frames5"].cpu().numpy()
    print(f"tower profile: frames differ by {np.abs(got_f5 - f5[which]).max(axis=0)}, tol {tol:.3e}, z0 tol {tol_z0:.3e}")
    assert np.abs(got_f5[:, [0, 1, 3, 4]] - f5[which][:, [0, 1, 3, 4]]).max() <= tol
    assert np.abs(got_f5[:, 2] - z0[which]).max() <= tol_z0 and np.array_equal(got_f5[:, 2], T["ground"])
    # both margins for the z0 actually used, so that everything integer may be compared exactly
    excess, boundary = tp.margins(R, perm, offsets, f5, slot, 3, dz, B)
    print(f"tower profile: excess margin {excess:.4f} m, boundary margin {boundary:.3e} m")
    # (a width moves by at most 2 tol, a row's height above z0 by at most tol_z0; ten times that, as terrain_cases asks)
    assert excess > 10.0 * 2.0 * tol and boundary > 10.0 * tol_z0
    assert np.array_equal(prof["count"].cpu().numpy(), want[0]) and np.array_equal(prof["outside"].cpu().numpy(), want[2])
    ext = prof["ext"].cpu().numpy()
    has = want[0] > 0
    assert np.array_equal(np.isinf(ext), np.isinf(want[1])) and np.abs(ext[has] - want[1][has]).max() <= tol
    # the levels: everything integer is the reference's; z_low, z_high and top are the reference's slices above the
    # z0 the device sampled (which lies within tol_z0 of the reference's)
    lv = tp.levels_reference(want[0], want[1], got_f5[:, 2], dz, ground=got_f5[:, 2])
    assert np.array_equal(T["n_levels"], lv["n_levels"]) and (T["n_levels"] == 1).all()
    for key in ("z_low", "z_high", "top", "rows", "tower_height", "nominal_height"):
        assert tc.same(T[key], lv[key]), key
    assert np.array_equal(np.isnan(T["width"]), np.isnan(lv["width"]))
    assert np.abs(T["width"][:, 0] - lv["width"][:, 0]).max() <= 2.0 * tol
    # the model's worst error at the tower feet is 0.5 m
    station = (got_f5[:, 0] + s["centroid"][0]) * np.cos(np.radians(sp.LINE_AZIMUTH_DEG)) + \
        (got_f5[:, 1] + s["centroid"][1]) * np.sin(np.radians(sp.LINE_AZIMUTH_DEG))
    tower = np.array([int(np.abs(np.array(sp.LINE_STATIONS) - v).argmin()) for v in station])
    base = np.array(sp.LINE_BASES)[tower]
    print(f"tower profile: nominal {T['nominal_height']}, height {T['tower_height']}, ground error "
          f"{T['ground'] + s['centroid'][2] - base}, lowest wire {T['lowest_wire']}")
    assert sorted(tower.tolist()) == [0, 1, 2]
    assert np.abs(T["nominal_height"] - tp.ARM_LOW).max() <= dz + 0.5
    assert np.abs(T["tower_height"] - tp.TOWER_TOP).max() <= dz + 0.5
    # lowest_wire: the height of the accepted pieces' curves at their ends within reach of the true axis, looped, above
    # the true base - within the model's 0.5 m; every tower holds the ends of three or six conductors, attached 21 m up
    sd = s["spans"]
    acc = sd["accepted"].cpu().numpy()
    curves = ops.span_curves(sd["table"], sd["frames"], sd["ext"]).cpu().numpy()[acc]
    axis = sp.line_towers()[tower] - s["centroid"].astype(np.float64)
    assert acc.sum() == 6
    for i in range(3):
        heights = []
        for cx, cy, cz, ux, uy, a, b, c, m0, m1 in curves:
            for m in (m0, m1):
                if np.hypot(cx + m * ux - axis[i, 0], cy + m * uy - axis[i, 1]) <= 11.0:      # (all ends lie within 9.5)
                    heights.append(cz + a + m * (b + c * m))
        assert len(heights) in (3, 6), (i, heights)
        assert abs(T["lowest_wire"][i] - (min(heights) - axis[i, 2])) <= 0.5 + 1e-9, (i, heights)
        assert 17.5 < T["lowest_wire"][i] < 22.0
    # without terrain: the ground is where the cluster begins, stage B's threshold
    bare = pipeline.tower_profile(s["out"], which=which, dz=dz)
    assert bare["table"]["ground_from"] == ["cluster"] * 3 and torch.isnan(bare["table"]["lowest_wire"]).all()
    zmin = np.array([R[perm[offsets[k]:offsets[k + 1]], 2].min() for k in which], dtype=np.float64)
    assert np.array_equal(bare["table"]["ground"].cpu().numpy(), zmin)
    f5c = tp.frames5_of(frames, np.array([R[perm[offsets[k]:offsets[k + 1]], 2].min() if offsets[k + 1] > offsets[k]
                                          else 0.0 for k in range(K)], dtype=np.float64))
    wantc = tp.slices_reference(R, perm, offsets, f5c, slot, 3, dz, B)
    assert np.array_equal(bare["count"].cpu().numpy(), wantc[0]) and (bare["outside"].cpu().numpy()[:, 0] == 0).all()
    # all clusters, none, and the refusals
    every = pipeline.tower_profile(s["out"], terrain=s["terrain"], dz=dz)
    assert every["count"].shape == (K, B) and np.array_equal(every["count"].cpu().numpy()[which], want[0])
    none = pipeline.tower_profile(s["out"], which=[], terrain=s["terrain"], spans=s["spans"], dz=dz)
    assert none["count"].shape == (0, B) and none["table"]["ground_from"] == [] and none["table"]["z_low"].shape == (0, 8)
    with pytest.raises(ValueError, match="256"):
        pipeline.tower_profile(s["out"], dz=0.25, height=64.5)
    for bad in ([2, 1], [0, 0], [-1], [K]):
        with pytest.raises(ValueError):
            pipeline.tower_profile(s["out"], which=bad)
    with pytest.raises(ValueError, match="4096"):
        pipeline.tower_profile(dict(s["out"], nclusters=5000), which=np.arange(4097))


# ------------------------------------------------------------------ drop-in
def test_drop_in_knob_writes_the_tower_profile_table(cuda, tmp_path, monkeypatch):
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

    def run():
        logs = []
        return te.extract_towers(path, log_callback=logs.append, min_points=20), logs

    files = lambda: sorted(f.name for f in (tmp_path / "output_towers").iterdir())
    assert te.TOWER_PROFILE is None and te.SPANS is None and te.TERRAIN is None
    off, off_logs = run()
    off_files = files()
    table = tmp_path / "output_towers" / "tower_profile_info.csv"
    assert len(off) == 3 and not table.exists()
    monkeypatch.setattr(te, "TOWER_PROFILE", te.tower_profile_from_env("0.5"))
    on, logs = run()
    extra = [m for m in logs if "杆塔剖面" in m]
    assert len(extra) == 1 and "杆塔 3" in extra[0] and "有横担 3" in extra[0], extra
    assert [m for m in logs if "杆塔剖面" not in m] == off_logs
    assert files() == sorted(off_files + ["tower_profile_info.csv"])
    assert len(on) == len(off)
    for a, b in zip(on, off):                                                  # the tower dicts are the same
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    with open(table, newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == te.TOWER_PROFILE_COLUMNS and len(lines) == 1 + 3
    col = {name: [v[i] for v in lines[1:]] for i, name in enumerate(te.TOWER_PROFILE_COLUMNS)}
    assert all(v.startswith("tower_") for v in col["ID"]) and len(set(col["ID"])) == 3
    assert col["ground_from"] == ["cluster"] * 3 and col["n_levels"] == ["1"] * 3
    assert all(np.isnan(float(v)) for v in col["lowest_wire"])
    # the axes are the scene's, the cluster begins at stage B's threshold 3.5 m above the towers' feet at the lowest
    axes = np.array([[float(x), float(y)] for x, y in zip(col["x"], col["y"])])
    d = np.linalg.norm(axes[:, None, :] - sp.line_towers()[None, :, :2], axis=2)
    assert sorted(d.argmin(axis=1).tolist()) == [0, 1, 2] and d.min(axis=1).max() < 0.5
    base = np.array(sp.LINE_BASES)[d.argmin(axis=1)] + 3.5
    for i in range(3):
        low, high, width = (float(v) for v in col["levels"][i].split(";")[0].split(":"))
        g = float(col["ground_z"][i])
        assert base[i] - 1e-3 <= g <= base[i] + 3.6                            # (the feet below the threshold are cut)
        # the level begins with the slice that holds the arm's lower edge, or with the next one where that slice holds
        # too little of the arm to count
        assert abs(low - (base[i] + tp.ARM_LOW)) < 0.5 and abs(high - (base[i] + 27.0)) <= 0.5 and 15.5 < width < 16.5
        assert abs(float(col["nominal_height"][i]) - (low - g)) < 1e-9
        assert abs(float(col["tower_height"][i]) + g - (base[i] + tp.TOWER_TOP)) <= 0.5
    # with the spans and the terrain on, the ground is the model's and the wires are found
    monkeypatch.setattr(te, "SPANS", te.spans_from_env("1,5,9,20"))
    monkeypatch.setattr(te, "TERRAIN", te.terrain_from_env("1,12,0.5,7", spans=True))
    _, logs = run()
    assert any("杆塔剖面" in m and "地形地面 3" in m for m in logs)
    with open(table, newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    col = {name: [v[i] for v in lines[1:]] for i, name in enumerate(te.TOWER_PROFILE_COLUMNS)}
    assert col["ground_from"] == ["terrain"] * 3
    axes = np.array([[float(x), float(y)] for x, y in zip(col["x"], col["y"])])
    feet = np.array(sp.LINE_BASES)[np.linalg.norm(axes[:, None, :] - sp.line_towers()[None, :, :2], axis=2).argmin(axis=1)] + 3.5
    for i in range(3):
        # the sheet lies between 0 and 0.2 m, the towers' feet hang above it: heights are measured from the sheet; the
        # conductors are attached 21 m above the feet and have sagged by less than 3 m nine metres out
        assert -0.01 < float(col["ground_z"][i]) < 0.21
        assert feet[i] + tp.ARM_LOW - 0.5 - 0.21 <= float(col["nominal_height"][i]) <= feet[i] + tp.ARM_LOW + 0.5 + 0.01
        assert feet[i] + 18.0 - 0.21 < float(col["lowest_wire"][i]) < feet[i] + 21.5
    for name in ("tower_profile_info.csv", "spans_info.csv", "ground_clearance_info.csv"):
        (tmp_path / "output_towers" / name).unlink()
    monkeypatch.setattr(te, "TOWER_PROFILE", None)
    monkeypatch.setattr(te, "SPANS", None)
    monkeypatch.setattr(te, "TERRAIN", None)
    again, again_logs = run()
    assert again_logs == off_logs and len(again) == 3 and files() == off_files
