"""Conductor spans, host side: the numpy references (span_cases) against independent statements, the scenes the
row-for-row GPU tests stand on and their margins, the summation bound, the frame and fit arithmetic of ops on host
tensors, the drop-in's knob and the C ABI's names.  No GPU."""
import os
import re

import numpy as np
import pytest

import shape_cases as sc
import span_cases as sp
from pointcloudhookup_amd import _lib, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("pch_cluster_moments_ws_bytes", "pch_cluster_moments_f32", "pch_cluster_profile_ws_bytes",
               "pch_cluster_profile_f32")


def _random_grouping(rng, sizes, noise=0):
    """rows scattered over a file of sum(sizes) + noise rows, cluster k owning sizes[k] of them"""
    n = int(sum(sizes)) + noise
    labels = np.full(n, -1, dtype=np.int32)
    order = rng.permutation(n)
    at = 0
    for k, m in enumerate(sizes):
        labels[order[at:at + m]] = k
        at += m
    return labels, sp.group_reference(labels, len(sizes))


# ------------------------------------------------------------------ (a) the references against independent statements
def test_moments_and_frames_against_np_cov():
    rng = np.random.default_rng(11)
    sizes = [1, 2, 3, 50, 0, 700]
    labels, (perm, offsets) = _random_grouping(rng, sizes, noise=20)
    az = np.radians([0.0, 10.0, 80.0, -35.0, 0.0, 20.0])
    P = np.zeros((len(labels), 3))
    for k, m in enumerate(sizes):
        s = rng.uniform(-30.0, 30.0, m)
        P[labels == k] = np.stack([s * np.cos(az[k]), s * np.sin(az[k]), 0.002 * s * s], axis=1) \
            + rng.normal(0.0, 0.05, (m, 3))
    P = (P + np.array([437000.0, 3139000.0, 80.0])).astype(np.float32)   # projected-CRS scale
    count, origin, M, A = sp.moments_reference(P, perm, offsets)
    assert count.tolist() == sizes and (A >= np.abs(M)).all()
    F = sp.frames_reference(count, origin, M)
    for k, m in enumerate(sizes):
        rows = np.flatnonzero(labels == k)
        if m == 0:
            assert not M[k].any() and not origin[k].any() and F[k].tolist() == [0, 0, 0, 1, 0, 1]
            continue
        assert np.array_equal(origin[k], P[rows[0]])                     # the first row in file order
        X = P[rows].astype(np.float64)
        assert np.abs(F[k, :3] - X.mean(0)).max() <= 1e-9
        if m < 3:
            continue
        C = np.cov(X[:, :2] - X[0, :2], rowvar=False, bias=True)
        w, V = np.linalg.eigh(C)
        u = V[:, 1] if V[0, 1] > 0 else -V[:, 1]
        assert abs(F[k, 3] * u[1] - F[k, 4] * u[0]) <= 1e-9              # the same axis
        assert F[k, 3] > 0 and abs(1.0 / F[k, 5] - np.sqrt(3.0 * w[1])) <= 1e-9 * np.sqrt(w[1])
        if m >= 50:                                                      # rows spread evenly: h is half the length
            assert abs(np.degrees(np.arctan2(F[k, 4], F[k, 3])) - np.degrees(az[k])) < 1.0
            assert abs(1.0 / F[k, 5] - 30.0) < 3.0


def test_fit_against_lstsq_within_the_normal_equations_error():
    rng = np.random.default_rng(12)
    sizes = [3, 40, 900]
    labels, (perm, offsets) = _random_grouping(rng, sizes)
    P = np.zeros((len(labels), 3))
    for k, m in enumerate(sizes):
        s = rng.uniform(-25.0, 25.0, m)
        P[labels == k] = np.stack([s, 0.3 * s, 5.0 + 0.01 * s + 0.003 * s * s], axis=1) + rng.normal(0, 0.02, (m, 3))
    P = P.astype(np.float32)
    count, origin, M, _ = sp.moments_reference(P, perm, offsets)
    F = sp.frames_reference(count, origin, M)
    S, E, _ = sp.profile_reference(P, perm, offsets, F)
    T = sp.fit_reference(count, F, S, E)
    for k in range(len(sizes)):
        _, s, dz = sp.profile_terms(P, perm[offsets[k]:offsets[k + 1]], F[k])
        Amat = np.stack([np.ones_like(s), s, s * s], axis=1)
        x = np.linalg.lstsq(Amat, dz, rcond=None)[0]
        cond = np.linalg.cond(Amat)
        h = 1.0 / F[k, 5]
        got = np.array([T["a"][k], T["b"][k] * h, T["c"][k] * h * h])
        bound = 64.0 * sp.U * cond * cond * np.linalg.norm(x)
        print(f"n = {sizes[k]}: cond2(A) = {cond:.3f}, |x - lstsq| = {np.abs(got - x).max():.3e}, bound {bound:.3e}")
        assert np.abs(got - x).max() <= bound
        assert abs(T["cond"][k] - cond * cond) <= 1e-9 * cond * cond      # cond2(G) = cond2(A)^2
        if sizes[k] > 3:
            p = np.polyfit(s, dz, 2)
            assert np.abs(got - p[::-1]).max() <= 1e-9
            res = dz - Amat @ x
            assert abs(T["rms_z"][k] - np.sqrt((res * res).mean())) <= 1e-9
        assert E[k].tolist() == [s.min(), s.max(), dz.min(), dz.max()]
        assert abs(T["length"][k] - (s.max() - s.min()) * h) <= 1e-12 * h
    assert 13.0 < T["cond"][2] < 16.0                                     # s scaled to about [-1, 1]: about 14
    assert abs(T["c"][2] - 0.003 / (1.0 + 0.09)) < 1e-4                   # per metre of along-track distance


def test_fit_rejects_short_and_singular_pieces():
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [0, 0, 2], [0, 0, 3]], dtype=np.float32)
    perm = np.arange(5, dtype=np.int32)
    offsets = np.array([0, 2, 5, 5], dtype=np.int64)                      # two rows, a vertical line, nothing
    count, origin, M, _ = sp.moments_reference(P, perm, offsets)
    F = sp.frames_reference(count, origin, M)
    S, E, _ = sp.profile_reference(P, perm, offsets, F)
    T = sp.fit_reference(count, F, S, E)
    for key in ("a", "b", "c", "sag", "z_low", "rms_z"):
        assert np.isnan(T[key]).all()
    assert T["length"].tolist() == [1.0, 0.0, 0.0] and E[2].tolist() == [np.inf, -np.inf, np.inf, -np.inf]
    acc = (T["length"] >= 0.0) & (T["rms_z"] <= 1.0) & (T["rms_t"] <= 1.0)
    assert not acc.any()                                                  # NaN is never accepted


def test_ops_frame_and_fit_arithmetic_on_host_tensors():
    """ops.span_frames and ops.span_fit are torch arithmetic on K records; the same arithmetic on host tensors agrees
    with the references within the table bound"""
    import torch
    r = sp.reference("line_cut")
    X = sp.line_scene()[0][r["wire"]]
    count, origin, M, _ = sp.moments_reference(X, r["perm"], r["offsets"])
    F = ops._span_frames_of(torch.from_numpy(count), torch.from_numpy(origin), torch.from_numpy(M)).numpy()
    assert np.abs(F - r["frames"]).max() <= 1e-12
    T = ops._span_fit_of(torch.from_numpy(count), torch.from_numpy(r["frames"]), torch.from_numpy(r["sums"]),
                         torch.from_numpy(r["ext"]))
    assert tuple(T) == sp.TABLE_KEYS == ops.SPAN_TABLE_KEYS
    bound = sp.table_bounds(r["table"])
    for key in sp.TABLE_KEYS:
        got, want = T[key].numpy().astype(np.float64), np.asarray(r["table"][key], dtype=np.float64)
        diff = np.abs(got - want).reshape(len(bound), -1).max(1)
        assert (diff <= bound).all(), (key, diff, bound)
    # the short, the singular and the empty piece
    P = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [0, 0, 2], [0, 0, 3]], dtype=np.float32)
    perm, offsets = np.arange(5, dtype=np.int32), np.array([0, 2, 5, 5], dtype=np.int64)
    count, origin, M, _ = sp.moments_reference(P, perm, offsets)
    Fr = sp.frames_reference(count, origin, M)
    F = ops._span_frames_of(torch.from_numpy(count), torch.from_numpy(origin), torch.from_numpy(M)).numpy()
    assert np.array_equal(F, Fr)
    S, E, _ = sp.profile_reference(P, perm, offsets, Fr)
    T = ops._span_fit_of(torch.from_numpy(count), torch.from_numpy(Fr), torch.from_numpy(S), torch.from_numpy(E))
    want = sp.fit_reference(count, Fr, S, E)
    for key in sp.TABLE_KEYS:
        assert np.allclose(T[key].numpy(), want[key], rtol=0, atol=1e-12, equal_nan=True), key


# ------------------------------------------------------------------ (b) the scenes are fit for a row-for-row test
def _margins(r, cut_radius=None):
    f = r["features"]
    assert np.abs(f["linearity"] - sc.SCENE_RULE["linearity"]).min() > 1e-9
    assert np.abs(f["verticality"] - sc.SCENE_RULE["verticality"]).min() > 1e-9
    assert not (r["neighbours"] == 0).any()
    if cut_radius is not None:
        assert np.abs(np.sqrt(r["tower_d2"]) - cut_radius).min() > 1e-9


def test_scene_gives_three_pieces_with_the_generating_curve():
    X, wire, _ = sc.scene()
    r = sp.reference("scene")
    _margins(r)
    assert r["wire"].sum() == 1657 and not (r["wire"] & ~wire).any()
    T = r["table"]
    assert r["nclusters"] == 3 and T["count"].tolist() == [555, 558, 544] and r["accepted"].all()
    assert np.abs(T["c"] - 3.0 / 900.0).max() < 2e-5                      # z = 26 - 3(1 - (x/30 - 1)^2)
    assert (T["rms_z"] > 0.018).all() and (T["rms_z"] < 0.021).all()
    assert np.abs(T["cond"] - 14.13).max() < 0.02
    assert np.abs(T["z_low"] - 23.0).max() < 0.01 and np.abs(T["azimuth_deg"]).max() < 0.01
    assert sorted(np.round(T["centre"][:, 1]).tolist()) == [-7.0, 0.0, 7.0]


def test_line_scene_without_towers_rejects_the_through_conductors():
    X, kind = sp.line_scene()
    assert X.shape == (sp.LINE_ROWS, 3) and X.dtype == np.float32
    r = sp.reference("line")
    _margins(r)
    assert r["wire"].sum() == 4440 and not r["wire"][(kind == 0) | (kind == 7)].any()
    T = r["table"]
    through = T["count"] == 1502                                          # the outer conductors run past the middle tower
    assert through.sum() == 2 and (np.abs(T["length"][through] - 150.0) < 0.1).all()
    assert (T["rms_z"][through] > 0.5).all() and not r["accepted"][through].any()
    assert r["accepted"].sum() == 2                                       # the centre conductor, cut by the tower bodies


def test_line_scene_with_towers_gives_six_spans_and_rejects_the_bar():
    X, kind = sp.line_scene()
    r = sp.reference("line_cut")
    _margins(r, 9.0)
    T = r["table"]
    assert r["nclusters"] == 7 and r["accepted"].sum() == 6
    lab = np.full(len(X), -2)
    lab[r["wire"]] = r["labels"]
    seen = set()
    for k in range(7):
        kinds = np.unique(kind[lab == k])
        assert len(kinds) == 1                                            # one conductor of one span, or the bar
        seen.add(int(kinds[0]))
        if kinds[0] == 8:
            assert not r["accepted"][k] and T["count"][k] == 61 and T["length"][k] < 7.0
            continue
        span = (int(kinds[0]) - 1) // 3
        assert r["accepted"][k] and 51.8 <= T["length"][k] <= 66.6          # this generator: 51.87 to 66.56 m
        want = 4.0 * sp.LINE_SAGS[span] / (sp.LINE_STATIONS[span + 1] - sp.LINE_STATIONS[span]) ** 2
        assert abs(T["c"][k] - want) < 2e-5                               # 4·sag/L²: 0.00125 and 0.00204
        assert abs(T["azimuth_deg"][k] - sp.LINE_AZIMUTH_DEG) < 0.01
        assert T["rms_z"][k] < 0.022 and T["rms_t"][k] < 0.022 and abs(T["cond"][k] - 14.13) < 0.02
    assert seen == {1, 2, 3, 4, 5, 6, 8}


# ------------------------------------------------------------------ (c) the summation bound
def test_two_summation_orders_stay_inside_the_bound():
    rng = np.random.default_rng(13)
    r = sp.reference("line_cut")
    X = sp.line_scene()[0][r["wire"]] + np.array([437000.0, 3139000.0, 80.0], dtype=np.float32)
    perm, offsets = r["perm"], r["offsets"]
    count, origin, M, A = sp.moments_reference(X, perm, offsets)
    F = sp.frames_reference(count, origin, M)
    S, E, AS = sp.profile_reference(X, perm, offsets, F)
    worst = 0.0
    for k in range(len(count)):
        rows = perm[offsets[k]:offsets[k + 1]]
        d = X[rows].astype(np.float64) - origin[k].astype(np.float64)
        t1 = (d[:, 0], d[:, 1], d[:, 2], d[:, 0] ** 2, d[:, 1] ** 2, d[:, 2] ** 2, d[:, 0] * d[:, 1], d[:, 0] * d[:, 2],
              d[:, 1] * d[:, 2])
        t3 = sp.profile_terms(X, rows, F[k])[0]
        for terms, ref, bound in ((t1, M[k], sp.sum_bounds(count[k:k + 1], A[k:k + 1])[0]),
                                  (t3, S[k], sp.sum_bounds(count[k:k + 1], AS[k:k + 1])[0])):
            for a, t in enumerate(terms):
                order = rng.permutation(len(t))
                seq = 0.0
                for v in t[order]:                                        # a sequential sum in another order
                    seq = seq + v
                blocks = sum(float(t[i:i + 64].sum()) for i in range(0, len(t), 64))
                for other in (seq, blocks):
                    assert abs(other - ref[a]) <= bound[a]
                    if bound[a] > 0:
                        worst = max(worst, abs(other - ref[a]) / bound[a])
    print(f"worst share of the summation bound: {worst:.3f}")


# ------------------------------------------------------------------ the drop-in's knob
def test_spans_knob_parses_and_validates():
    from pointcloudhookup_amd.utils import tower_extraction as te
    assert te.spans_from_env(None) is None and te.spans_from_env("  ") is None
    assert te.spans_from_env("1, 5,9,20") == dict(eps=1.0, min_rows=5, cut_radius=9.0, min_length=20.0)
    for bad in ("1,5,9", "1,5,9,20,3", "0,5,9,20", "nan,5,9,20", "1,0,9,20", "1,5,-1,20", "1,5,9,inf", "1,5.5,9,20",
                "a,b,c,d"):
        with pytest.raises(ValueError):
            te.spans_from_env(bad)


# ------------------------------------------------------------------ (d) symbols and workspace
def test_new_symbols_are_declared_bound_and_size_their_workspace():
    header = open(os.path.join(ROOT, "include", "pch_hip.h")).read()
    declared = set(re.findall(r"\b(pch_[a-z0-9_]+)\s*\(", header))
    assert set(NEW_SYMBOLS) <= declared and set(NEW_SYMBOLS) <= set(_lib.exported_symbols())
    L = _lib.lib()
    for name in ("pch_cluster_moments_ws_bytes", "pch_cluster_profile_ws_bytes"):
        fn = getattr(L, name)
        assert fn(0, 0) > 0 and fn(1, 1) > 0
        assert fn(10 ** 7, 1) < 16 * 10 ** 7 // 32                        # one 128-byte partial per 512 rows and cluster
        assert fn(-1, 1) == 0 and fn(1, -1) == 0
    for fn in (ops.cluster_moments, ops.cluster_profile):
        with pytest.raises(TypeError):
            fn(np.zeros((3, 3), np.float32), np.zeros(3, np.int32), np.zeros(2, np.int64), 1, *([None] * (fn is ops.cluster_profile)))
    import torch
    with pytest.raises(TypeError):
        ops.span_frames(torch.zeros(1, dtype=torch.int64), torch.zeros(1, 3), torch.zeros(1, 9, dtype=torch.float64))
    with pytest.raises(TypeError):
        ops.span_fit(torch.zeros(1, dtype=torch.int64), torch.zeros(1, 6, dtype=torch.float64),
                     torch.zeros(1, 10, dtype=torch.float64), torch.zeros(1, 4, dtype=torch.float64))
