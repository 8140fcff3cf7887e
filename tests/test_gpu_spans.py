"""Conductor spans on the device: the two segmented reductions (pch_cluster_moments_f32, pch_cluster_profile_f32) against
the numpy statement of span_cases at the smallest shapes that can go wrong, and pipeline.conductor_spans and the
drop-in's PCH_SPANS against the reference row for row.  count, origin and the extrema are demanded bit for bit, every
sum inside span_cases.sum_bounds; the worst share of the bound is printed per case."""
import csv

import numpy as np
import pytest
import torch

import las_bytes
import shape_cases as sc
import span_cases as sp
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

BLOCK = 512                                      # entries of perm per wave (SP_BLOCK of pch_spans.hip)
EPSG = np.array([437000.0, 3139000.0, 80.0])


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)               # (a copy: the scenes are read-only)


def _case(sizes, noise=0, seed=0, shift=None):
    """(P float32 [n,3], perm, offsets): cluster k is a noisy sagging line of sizes[k] rows at its own azimuth, its rows
    scattered over a file of sum(sizes) + noise rows"""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes)) + noise
    labels = np.full(n, -1, dtype=np.int32)
    order = rng.permutation(n)
    P = rng.uniform(-50.0, 50.0, (n, 3))
    at = 0
    for k, m in enumerate(sizes):
        rows = order[at:at + m]
        at += m
        labels[rows] = k
        s = rng.uniform(-20.0, 20.0, m)
        az = rng.uniform(-1.5, 1.5)
        P[rows] = np.stack([s * np.cos(az), s * np.sin(az), 0.004 * s * s], axis=1) + rng.normal(0.0, 0.05, (m, 3)) \
            + rng.uniform(-30.0, 30.0, 3)
    if shift is not None:
        P = P + shift
    perm, offsets = sp.group_reference(labels, len(sizes))
    return P.astype(np.float32), perm, offsets


def _share(got, want, bound):
    diff = np.abs(got - want)
    assert (diff <= bound).all(), (np.argwhere(diff > bound)[:5], diff.max())
    nz = bound > 0
    return float((diff[nz] / bound[nz]).max()) if nz.any() else 0.0


def _run(P, perm, offsets, cuda):
    K = len(offsets) - 1
    dP, dperm, doff = _dev(P, cuda), _dev(perm, cuda), _dev(offsets, cuda)
    count, origin, M = ops.cluster_moments(dP, dperm, doff, K)
    rc, ro, rM, rA = sp.moments_reference(P, perm, offsets)
    F = sp.frames_reference(rc, ro, rM)                                   # the reference's frames feed the profile
    S, E = ops.cluster_profile(dP, dperm, doff, K, _dev(F, cuda))
    return (count.cpu().numpy(), origin.cpu().numpy(), M.cpu().numpy(), S.cpu().numpy(), E.cpu().numpy()), \
        (rc, ro, rM, rA, F)


def _check(P, perm, offsets, cuda, what):
    (count, origin, M, S, E), (rc, ro, rM, rA, F) = _run(P, perm, offsets, cuda)
    rS, rE, rAS = sp.profile_reference(P, perm, offsets, F)
    assert count.dtype == np.int64 and np.array_equal(count, rc), what
    assert np.array_equal(origin.view(np.uint32), ro.view(np.uint32)), what
    assert np.array_equal(E.view(np.uint64), rE.view(np.uint64)), what
    s1 = _share(M, rM, sp.sum_bounds(rc, rA))
    s3 = _share(S, rS, sp.sum_bounds(rc, rAS))
    print(f"{what}: K = {len(rc)}, rows = {len(perm)}, worst share of the bound: moments {s1:.3f}, profile {s3:.3f}")
    return count, origin, M, S, E


# ------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65])
def test_one_cluster_of_a_few_rows(cuda, n):
    _check(*_case([n], seed=n), cuda, f"one cluster of {n}")


@pytest.mark.parametrize("n", [BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK])
def test_cluster_ending_on_a_block_boundary(cuda, n):
    _check(*_case([n, 70], seed=n), cuda, f"first cluster of {n} rows, then 70")
    _check(*_case([37, n - 37, 9], seed=n + 1), cuda, f"second cluster ends at entry {n}")


# sp_finish_k folds sixteen partials per buffer: its double-buffered loop runs from 48 partials on, the short trips
# behind it once, twice or three times; a cluster behind 37 other rows starts inside block 0, so its first slot is 1
@pytest.mark.parametrize("partials", [16, 17, 32, 33, 47, 48, 49, 100])
def test_cluster_of_many_blocks(cuda, partials):
    _check(*_case([partials * BLOCK], seed=partials), cuda, f"{partials} whole blocks")
    count, *_ = _check(*_case([37, (partials - 1) * BLOCK + 100, 9], noise=3, seed=100 + partials), cuda,
                       f"{partials} blocks, the first and the last in part")
    assert -(-(37 + count[1]) // BLOCK) == partials


SMALL = [1, 2, 3, 1, 2, 5, 1, 2, 4, 1] * 20         # 200 clusters of 1 to 5 rows, 440 rows: all inside one block


def test_long_cluster_beside_two_hundred_small_ones(cuda):
    assert len(SMALL) == 200 and sum(SMALL) < BLOCK and set(SMALL) == {1, 2, 3, 4, 5}
    # block 0 holds all 200 (four rounds of 64 looked-up clusters) and the head of the long one
    count, *_ = _check(*_case(SMALL + [3 * BLOCK + 77], noise=40, seed=7), cuda,
                       "200 clusters of 1 to 5 rows in one block, then three blocks and more")
    assert count.max() == 3 * BLOCK + 77 and len(count) == 201
    # and behind the long one, where they may straddle a block boundary
    _check(*_case(SMALL[:100] + [3 * BLOCK + 77] + SMALL[100:], noise=40, seed=8), cuda,
           "100 small clusters on either side of the long one")


def test_empty_clusters_first_last_and_adjacent(cuda):
    count, origin, M, S, E = _check(*_case([0, 0, 5, 0, 0, 0, 700, 0, 64, 0], seed=3), cuda, "empty clusters")
    empty = count == 0
    assert empty.sum() == 7 and not M[empty].any() and not origin[empty].any() and not S[empty].any()
    assert (E[empty] == np.array([np.inf, -np.inf, np.inf, -np.inf])).all()
    _check(*_case([0, 0, 0], noise=10, seed=4), cuda, "nothing but empty clusters and noise")
    _check(*_case([0], seed=5), cuda, "no rows at all")


def test_noise_rows_behind_the_last_cluster_belong_to_nobody(cuda):
    P, perm, offsets = _case([300, 100], noise=3 * BLOCK, seed=8)
    got = _check(P, perm, offsets, cuda, "noise behind the last cluster")
    P2 = P.copy()
    P2[perm[offsets[-1]:]] = np.float32(np.nan)                            # nobody's rows may hold anything
    again = _check(P2, perm, offsets, cuda, "NaN in the noise rows")
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_rows_at_projected_scale(cuda):
    _check(*_case([1, 700, 64, 1300], noise=5, seed=9, shift=EPSG), cuda, "EPSG-scale coordinates")


def test_nonfinite_rows_propagate(cuda):
    P, perm, offsets = _case([40, 50], seed=10)
    clean = sp.moments_reference(P, perm, offsets)
    F = sp.frames_reference(*clean[:3])                                    # finite frames for both clusters
    P[perm[5], 1] = np.float32(np.inf)
    P[perm[9], 2] = np.float32(np.nan)                                     # dz is NaN, s is not
    P[perm[17], 0] = np.float32(np.nan)                                    # s is NaN, dz is not
    (count, origin, M, _, _), (rc, ro, rM, rA, _) = _run(P, perm, offsets, cuda)
    assert np.array_equal(np.isnan(M), np.isnan(rM)) and np.array_equal(np.isinf(M), np.isinf(rM))
    assert not np.isfinite(M[0]).all() and np.isfinite(M[1]).all()             # the other cluster is untouched
    _share(M[1:], rM[1:], sp.sum_bounds(rc[1:], rA[1:]))
    assert np.array_equal(count, rc) and np.array_equal(origin.view(np.uint32), ro.view(np.uint32))
    # the profile in the clean frames: sums propagate, the extrema skip a NaN (include/pch_hip.h)
    S, E = ops.cluster_profile(_dev(P, cuda), _dev(perm, cuda), _dev(offsets, cuda), 2, _dev(F, cuda))
    S, E = S.cpu().numpy(), E.cpu().numpy()
    rS, rE, rAS = sp.profile_reference(P, perm, offsets, F)
    assert np.array_equal(np.isnan(S), np.isnan(rS)) and np.array_equal(np.isinf(S), np.isinf(rS))
    assert np.isnan(S[0]).any() and np.isfinite(S[1]).all()
    _share(S[1:], rS[1:], sp.sum_bounds(rc[1:], rAS[1:]))
    assert np.array_equal(E.view(np.uint64), rE.view(np.uint64))
    assert np.isfinite(E[0, 2:]).all() and np.isinf(E[0, :2]).sum() == 1       # NaN skipped, an infinite s is a value


def test_the_same_call_twice_gives_the_same_bits(cuda):
    P, perm, offsets = _case([5, 2000, 1, 3, 49 * BLOCK + 100, 800], noise=17, seed=11, shift=EPSG)   # 50 partials
    first, _ = _run(P, perm, offsets, cuda)
    second, _ = _run(P, perm, offsets, cuda)
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_refusals_and_the_raw_c_abi(cuda):
    L = _lib.lib()
    P, perm, offsets = _case([100, 30], noise=3, seed=12)
    n, K = len(perm), 2
    dP, dperm, doff = _dev(P, cuda), _dev(perm, cuda), _dev(offsets, cuda)
    count = torch.empty(K, dtype=torch.int64, device=cuda)
    origin = torch.empty((K, 3), dtype=torch.float32, device=cuda)
    M = torch.empty((K, 9), dtype=torch.float64, device=cuda)
    S = torch.empty((K, 10), dtype=torch.float64, device=cuda)
    E = torch.empty((K, 4), dtype=torch.float64, device=cuda)
    need = L.pch_cluster_moments_ws_bytes(n, K)
    assert need == L.pch_cluster_profile_ws_bytes(n, K) > 0
    ws = torch.empty(need, dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()

    def moments(out=None, cnt=None, org=None, w=ws, wb=None, nn=n, kk=K):
        return L.pch_cluster_moments_f32(p(dP), p(dperm), p(doff), nn, kk, p(count) if cnt is None else cnt,
                                         p(origin) if org is None else org, p(M) if out is None else out, p(w),
                                         need if wb is None else wb, st)

    assert moments() == 0
    rc, ro, rM, rA = sp.moments_reference(P, perm, offsets)
    assert np.array_equal(count.cpu().numpy(), rc) and np.array_equal(origin.cpu().numpy(), ro)
    _share(M.cpu().numpy(), rM, sp.sum_bounds(rc, rA))
    F = _dev(sp.frames_reference(rc, ro, rM), cuda)

    def profile(fr=None, out=None, ext=None, wb=None, nn=n, kk=K):
        return L.pch_cluster_profile_f32(p(dP), p(dperm), p(doff), nn, kk, p(F) if fr is None else fr,
                                         p(S) if out is None else out, p(E) if ext is None else ext, p(ws),
                                         need if wb is None else wb, st)

    assert profile() == 0
    before = [t.clone() for t in (count, origin, M, S, E)]
    assert moments(wb=need - 1) == -2 and profile(wb=need - 1) == -2       # PCH_ERR_WORKSPACE
    assert b"workspace" in L.pch_last_error()
    assert moments(kk=0) == 0 and profile(kk=0) == 0                       # no cluster: success, nothing written
    host = np.zeros((K, 10), dtype=np.float64)
    for rc_ in (moments(out=0), moments(cnt=0), moments(org=0), moments(nn=-1), moments(kk=-1),
                moments(out=host.ctypes.data), profile(out=0), profile(ext=0), profile(fr=0), profile(nn=-1),
                profile(out=host.ctypes.data)):
        assert rc_ == -1                                                   # PCH_ERR_ARG
    torch.cuda.synchronize()
    for t, b in zip((count, origin, M, S, E), before):
        assert torch.equal(t, b)                                           # a refused call writes nothing
    with pytest.raises(TypeError):
        ops.cluster_moments(P, dperm, doff, K)
    with pytest.raises(TypeError):
        ops.cluster_profile(dP, dperm, doff, K, F.cpu())
    with pytest.raises(ValueError):
        ops.cluster_moments(dP, dperm, doff, K + 1)
    with pytest.raises(TypeError):
        ops.span_frames(count.cpu(), origin, M)
    with pytest.raises(TypeError):
        ops.span_fit(count, F, S.cpu(), E)
    with pytest.raises(TypeError):
        pipeline.conductor_spans(torch.from_numpy(P))


# ------------------------------------------------------------------ pipeline level
def _table_check(out, ref, what):
    assert np.array_equal(out["wire"].cpu().numpy(), ref["wire"]), what
    assert out["nclusters"] == ref["nclusters"]
    assert np.array_equal(out["labels"].cpu().numpy(), ref["labels"]), what
    assert np.array_equal(out["perm"].cpu().numpy(), ref["perm"]) and np.array_equal(out["offsets"].cpu().numpy(),
                                                                                     ref["offsets"])
    assert np.array_equal(out["accepted"].cpu().numpy(), ref["accepted"]), what
    assert tuple(out["table"]) == sp.TABLE_KEYS
    bound = sp.table_bounds(ref["table"])
    worst = 0.0
    for key in sp.TABLE_KEYS:
        got = out["table"][key].cpu().numpy().astype(np.float64).reshape(len(bound), -1)
        want = np.asarray(ref["table"][key], dtype=np.float64).reshape(len(bound), -1)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (what, key)
        diff = np.nan_to_num(np.abs(got - want)).max(1) if got.size else np.zeros(0)
        assert (diff <= bound).all(), (what, key, diff, bound)
        worst = max(worst, float((diff / bound).max()) if len(bound) else 0.0)
    print(f"{what}: {ref['nclusters']} pieces, {int(ref['accepted'].sum())} accepted, worst share of the table bound "
          f"{worst:.3e}")


@pytest.mark.parametrize("name", ["scene", "scene_cut", "line", "line_cut"])
def test_conductor_spans_against_the_reference(cuda, name):
    base = name.split("_")[0]
    X = sc.scene()[0] if base == "scene" else sp.line_scene()[0]
    towers = None if not name.endswith("_cut") else (sp.scene_towers() if base == "scene" else sp.line_towers())
    out = pipeline.conductor_spans(_dev(X, cuda), rule=dict(sc.SCENE_RULE), towers=towers)
    _table_check(out, sp.reference(name), name)


def test_conductor_spans_without_wire_rows_and_without_a_grid(cuda):
    rng = np.random.default_rng(2)
    blob = rng.normal(0.0, 1.5, (500, 3)).astype(np.float32)
    out = pipeline.conductor_spans(_dev(blob, cuda))
    assert out["nclusters"] == 0 and not out["wire"].any() and out["labels"].numel() == 0
    assert out["accepted"].shape == (0,) and out["offsets"].tolist() == [0]
    assert tuple(out["table"]) == sp.TABLE_KEYS and all(v.shape[0] == 0 for v in out["table"].values())
    with pytest.raises(ValueError):
        pipeline.conductor_spans(_dev(blob[:0], cuda))
    wide = sc.scene()[0].copy()
    wide[0, 0] = np.float32(3.0e30)                                        # a grid beyond the 64-bit cell key
    with pytest.raises(RuntimeError, match="compressed"):
        pipeline.conductor_spans(_dev(wide, cuda))


def test_drop_in_knob_writes_the_span_table(cuda, tmp_path, monkeypatch):
    from pointcloudhookup_amd.utils import tower_extraction as te
    X, _ = sp.line_scene()
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

    assert te.SPANS is None
    off, off_logs = run()
    assert len(off) == 3 and not (tmp_path / "output_towers" / "spans_info.csv").exists()
    monkeypatch.setattr(te, "SPANS", te.spans_from_env("1,5,9,20"))
    on, logs = run()
    extra = [m for m in logs if "导线档距" in m]
    assert len(extra) == 1 and "接受 6" in extra[0], extra
    assert [m for m in logs if "导线档距" not in m] == off_logs
    assert len(on) == len(off)
    for a, b in zip(on, off):                                              # the tower dicts are the same
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    with open(tmp_path / "output_towers" / "spans_info.csv", newline="", encoding="utf-8") as f:
        lines = list(csv.reader(f))
    assert tuple(lines[0]) == te.SPANS_COLUMNS and len(lines) == 1 + 6
    col = {name: np.array([float(r[i]) for r in lines[1:]]) for i, name in enumerate(te.SPANS_COLUMNS) if i}
    c = np.sort(col["c"])
    assert np.abs(c[:3] - 4.0 * 2.0 / 80.0 ** 2).max() < 2e-5 and np.abs(c[3:] - 4.0 * 2.5 / 70.0 ** 2).max() < 2e-5
    assert np.abs(col["azimuth_deg"] - sp.LINE_AZIMUTH_DEG).max() < 0.01 and (col["length"] > 50.0).all()
    # world coordinates: the centres lie on the three conductors of the two spans, at the scene's heights plus the lift
    a = np.radians(sp.LINE_AZIMUTH_DEG)
    lateral = -col["x"] * np.sin(a) + col["y"] * np.cos(a)
    assert sorted(np.round(lateral).tolist()) == [-6.0, -6.0, 0.0, 0.0, 6.0, 6.0]
    assert (col["z"] > 20.0 + 3.5).all() and (col["z"] < 33.0 + 3.5).all() and (col["z_low"] < col["z"]).all()
    monkeypatch.setattr(te, "SPANS", None)
    again, again_logs = run()
    assert again_logs == off_logs and len(again) == 3
