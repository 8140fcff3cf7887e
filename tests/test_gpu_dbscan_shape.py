"""ops.DbscanFit.shape / pch_dbscan_shape_f32, ops.shape_features / pch_shape_features_f64 and the opt-in wire removal
built on them (pipeline.drop_linear_rows, cluster_points(drop_linear=...), the drop-in's DROP_LINEAR).

Every expectation is shape_cases.shape_reference, the all-pairs statement of the rule: counts are compared exactly,
moments within shape_cases.moment_bounds - with u = 2^-53 and n = count, 2(n+1)·u·n·r for the three first moments and
2(n+1)·u·n·r² for the six second moments, the distance two summation orders of the same terms can lie apart."""
import ctypes as C

import numpy as np
import pytest
import torch

import kdist_cases as kc
import las_bytes
import shape_cases as sc
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

PIECE = 8                    # DS_PIECE of pch_dbscan_query.hip: queries of one cell a wave takes at most


# ------------------------------------------------------------------ running
def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(cuda)       # a copy: cached inputs are read-only


def _shape(fit, Q, radius, cuda, sub=None, chunk=None):
    """(count, moments) of fit.shape on host arrays; the fit's labels and core flags must come out as they went in"""
    labels, core = fit.labels.clone(), fit.core.clone()
    if chunk is not None and not isinstance(chunk, str):
        chunk = _dev(np.asarray(chunk, dtype=np.int32), cuda)
    count, M = fit.shape(_dev(np.asarray(Q, dtype=np.float32).reshape(-1, 3), cuda), radius, sub=sub, chunk=chunk)
    assert count.dtype == torch.int32 and M.dtype == torch.float64 and count.is_cuda and M.is_cuda
    assert M.shape == (count.shape[0], 9)
    assert torch.equal(fit.labels, labels) and torch.equal(fit.core, core)
    return count.cpu().numpy(), M.cpu().numpy()


def _same(got, want, radius, what=""):
    """counts equal, moments within the bound; prints the worst share of the bound before it asserts"""
    count, M = got
    wc, wM = want
    np.testing.assert_array_equal(count, wc, err_msg=f"count {what}")
    B = sc.moment_bounds(wc, radius)
    diff = np.abs(M - wM)
    share = float((diff[B > 0] / B[B > 0]).max()) if (B > 0).any() else 0.0
    print(f"shape {what}: nq {len(wc)}, count {wc.min() if len(wc) else 0}..{wc.max() if len(wc) else 0}, "
          f"worst share of the moment bound {share:.4f}")
    assert (diff <= B).all(), what
    assert not M[wc == 0].any(), what                                         # nine zeros, not nearly zero


def _check(fit, X, Q, radius, cuda, chunk_size=0, qc=None, sub=None, what="", chunk=None):
    want = sc.shape_reference(X, Q, radius, chunk_size, qc, sub=sub)
    got = _shape(fit, Q, radius, cuda, sub=sub, chunk=qc if chunk is None else chunk)
    _same(got, want, radius, what)
    return want


_CLOUD = {}


def _cloud():
    """3000 rows: a clump, a plate and a uniform part in a 6 m box - neighbourhoods of 1 to some hundreds at eps = 1"""
    if not _CLOUD:
        rng = np.random.default_rng(21)
        X = np.vstack([rng.normal(3.0, 0.25, (900, 3)), rng.uniform(0.0, 6.0, (1500, 3)),
                       np.c_[rng.uniform(0.0, 6.0, (600, 2)), rng.normal(1.0, 0.02, 600)]]).astype(np.float32)
        X = X[rng.permutation(len(X))]
        Q = np.vstack([X[::5], (X[:300] + rng.normal(0.0, 0.2, (300, 3))).astype(np.float32)])
        X.setflags(write=False)
        Q.setflags(write=False)
        _CLOUD["case"] = (X, Q)
    return _CLOUD["case"]


# ------------------------------------------------------------------ a. nq, pieces, candidate totals
def test_nq_zero_and_one(cuda):
    X, Q = _cloud()
    fit = ops.DbscanFit(_dev(X, cuda), 1.0, 10)
    count, M = fit.shape(torch.empty((0, 3), dtype=torch.float32, device=cuda), 1.0)
    assert count.shape == (0,) and M.shape == (0, 9)
    _check(fit, X, X[17:18], 1.0, cuda, what="nq=1")


@pytest.mark.parametrize("nq", [1, PIECE, PIECE + 1, 65])
def test_pieces_of_one_cell(cuda, nq):
    """nq queries in one cell: a piece boundary at PIECE, the 64-query inner loop at 65"""
    X, _ = _cloud()
    rng = np.random.default_rng(nq)
    Q = (np.repeat(X[40:41], nq, axis=0) + rng.uniform(-1e-4, 1e-4, (nq, 3))).astype(np.float32)
    Q[: (nq + 1) // 2] = X[40]                                                # equal queries share a cell for certain
    fit = ops.DbscanFit(_dev(X, cuda), 1.0, 10)
    _check(fit, X, Q, 1.0, cuda, what=f"{nq} queries in one cell")
    _check(fit, X, np.vstack([Q, X[::50]]), 0.5, cuda, what=f"{nq} queries in one cell among others")


@pytest.mark.parametrize("T", [1, 63, 64, 65, 256, 257, 1500])
def test_candidate_totals(cuda, T):
    """a clump of T rows and nothing else: T candidates - the 64-candidate group edge, the four-groups-per-trip edge,
    several trips.  From 10 rows on the clump's cell holds >= min_samples rows (all core: no dense-cell shortcut may
    answer), and a query 3 eps away has an empty neighbourhood"""
    rng = np.random.default_rng(T)
    X = (np.float32(2.0) + rng.uniform(0.0, 0.05, (T, 3))).astype(np.float32)
    Q = np.vstack([X[: min(T, 5)], X[:1] + np.float32(0.4), X[:1] + np.array([1.1, 0, 0], dtype=np.float32),
                   X[:1] + np.array([3.0, 0, 0], dtype=np.float32), X[:1] - np.float32(1.2)]).astype(np.float32)
    fit = ops.DbscanFit(_dev(X, cuda), 1.0, 10)
    if T >= 10:
        assert bool(fit.core.all())
    want = _check(fit, X, Q, 1.0, cuda, what=f"T={T}")
    assert want[0][0] == T and (want[0][-3:] == 0).all()           # beside the clump, beyond the grid on either side


# ------------------------------------------------------------------ b. the radius as an edge
def test_lattice_ties_are_in_and_the_next_float_is_out(cuda):
    g = np.arange(-6, 7, dtype=np.float32)
    L = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    up = np.nextafter(np.float32(5.0), np.float32(np.inf))
    out = np.array([[3, np.nextafter(np.float32(4.0), np.float32(np.inf)), 0], [up, 0, 0], [0, 0, up],
                    [0, -up, 0]], dtype=np.float32)
    X = np.vstack([L, out])
    Q = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 1], [0.5, 0.5, 0.5]], dtype=np.float32)
    fit = ops.DbscanFit(_dev(X, cuda), 5.0, 10)
    want = _check(fit, X, Q, 5.0, cuda, what="lattice r=5")
    d2 = (L.astype(np.float64) ** 2).sum(1)
    assert (d2 == 25.0).sum() == 30 and want[0][0] == (d2 <= 25.0).sum()      # the 30 ties in, the four beyond out
    for tie in ((3, 4, 0), (5, 0, 0), (0, 0, 5)):
        P = np.vstack([np.array([tie], dtype=np.float32), out])
        got = _shape(ops.DbscanFit(_dev(P, cuda), 5.0, 1), Q[:1], 5.0, cuda)
        assert got[0][0] == 1 and np.array_equal(got[1][0, :3], np.array(tie, dtype=np.float64))


@pytest.mark.parametrize("part", [1.0, 0.25])
def test_radius_eps_and_a_quarter(cuda, part):
    X, Q = _cloud()
    fit = ops.DbscanFit(_dev(X, cuda), 1.0, 10)
    want = _check(fit, X, Q, part * 1.0, cuda, what=f"radius = {part} eps")
    assert want[0].max() > (64 if part == 1.0 else 4)                         # more than one group of candidates in range


def test_radius_beyond_eps_raises_and_the_fit_stays_usable(cuda):
    X, Q = _cloud()
    fit = ops.DbscanFit(_dev(X, cuda), 1.0, 10)
    q = _dev(Q[:10], cuda)
    with pytest.raises(ValueError):
        fit.shape(q, 1.0000001)
    L = _lib.lib()
    count = torch.empty((10,), dtype=torch.int32, device=cuda)
    M = torch.empty((10, 9), dtype=torch.float64, device=cuda)
    qws = torch.empty(int(L.pch_dbscan_shape_ws_bytes(10)) + 256, dtype=torch.uint8, device=cuda)
    for radius in (1.5, 0.0, -1.0, float("nan"), float("inf")):
        rc = L.pch_dbscan_shape_f32(q.data_ptr(), 10, None, None, radius, fit.n, count.data_ptr(), M.data_ptr(),
                                    qws.data_ptr(), qws.numel(), fit.workspace.data_ptr(), fit.workspace.numel(),
                                    torch.cuda.current_stream().cuda_stream)
        assert rc == -1, radius                                               # PCH_ERR_ARG
    assert "eps" in L.pch_last_error().decode() or "radius" in L.pch_last_error().decode()
    _check(fit, X, Q[:10], 1.0, cuda, what="after the refusals")


# ------------------------------------------------------------------ c. chunks, foreign queries, sub
def _chunked():
    rng = np.random.default_rng(33)
    X = np.vstack([rng.normal(2.0, 0.4, (1200, 3)), rng.uniform(0.0, 5.0, (1200, 3))]).astype(np.float32)
    return X[rng.permutation(len(X))]                                         # 2400 rows: 700, 700, 700, 300


def test_chunks_own(cuda):
    X = _chunked()
    fit = ops.DbscanFit(_dev(X, cuda), 1.0, 10, 700)
    assert fit.chunk_size == 700
    qc = (np.arange(len(X)) // 700).astype(np.int32)
    want = sc.shape_reference(X, X, 0.8, 700, qc)
    _same(_shape(fit, X, 0.8, cuda, chunk="own"), want, 0.8, "own, chunks of 700")
    _same(_shape(fit, X, 0.8, cuda, chunk=qc), want, 0.8, "the chunk tensor says the same")
    assert want[0].min() >= 1                                                 # every row finds itself


def test_foreign_queries_bad_chunks_and_nan_rows(cuda):
    X = _chunked()
    fit = ops.DbscanFit(_dev(X, cuda), 1.0, 10, 700)
    rng = np.random.default_rng(34)
    Q = (X[rng.choice(len(X), 400)] + rng.normal(0.0, 0.3, (400, 3))).astype(np.float32)
    Q[380:390] += np.float32(7.0)                                             # 7 eps away and further
    Q[5], Q[77, 1], Q[201, 2] = np.nan, np.inf, -np.inf
    qc = rng.integers(0, 4, 400).astype(np.int32)
    qc[::9] = -1
    qc[4::9] = 4                                                              # nchunks
    qc[8::45] = 2 ** 31 - 1
    want = _check(fit, X, Q, 1.0, cuda, 700, qc, what="foreign queries")
    assert (want[0][::9] == 0).all() and want[0][5] == 0 and (want[0][380:390] == 0).all() and want[0].max() > 50


def test_sub_given(cuda):
    X, Q = _cloud()
    sub = np.array([437000.5, 3139000.25, 12.125], dtype=np.float32)
    fit = ops.DbscanFit(_dev(X, cuda), 1.0, 10)
    Qw = (Q[:200] + sub).astype(np.float32)                                   # world coordinates: a coarser grid
    want = _check(fit, X, Qw, 1.0, cuda, sub=sub, what="sub")
    assert want[0].max() > 10


# ------------------------------------------------------------------ d. a neighbourhood of thousands
def test_big_cloud(cuda):
    X, rows = kc.big_cloud()
    fit = ops.DbscanFit(_dev(X, cuda), kc.BIG_EPS, 80)
    want = _check(fit, X, X[rows], kc.BIG_EPS, cuda, what="big cloud")
    assert want[0].max() >= 5000


# ------------------------------------------------------------------ e. labels play no part
def test_before_and_after_relabel(cuda):
    X, Q = _cloud()
    fit = ops.DbscanFit(_dev(X, cuda), 1.0, 10)
    q = _dev(Q, cuda)
    c0, m0 = fit.shape(q, 0.7)
    assert fit.nclusters >= 1
    fit.relabel(torch.arange(fit.nclusters - 1, -1, -1, dtype=torch.int32, device=cuda))
    c1, m1 = fit.shape(q, 0.7)
    assert torch.equal(c0, c1) and torch.equal(m0.view(torch.int64), m1.view(torch.int64))
    _same((c1.cpu().numpy(), m1.cpu().numpy()), sc.shape_reference(X, Q, 0.7), 0.7, "after relabel")


# ------------------------------------------------------------------ f. the solver alone
def _features(count, M, cuda):
    f = ops.shape_features(_dev(np.asarray(count, dtype=np.int32), cuda), _dev(np.asarray(M, dtype=np.float64), cuda))
    assert sorted(f) == ["l1", "l2", "l3", "linearity", "planarity", "scattering", "verticality"]
    assert all(v.dtype == torch.float64 and v.is_cuda for v in f.values())
    return {k: v.cpu().numpy() for k, v in f.items()}


def _solver_check(count, M, cuda, what):
    """eigenvalues within 2^-40 trace of np.linalg.eigvalsh (both solvers are backward stable to a small multiple of
    u·|C|); verticality within 2^-30 where l1 - l2 >= 2^-8 trace (Davis-Kahan: 2|E|/gap)"""
    got = _features(count, M, cuda)
    C, trace = sc.covariance(count, M)
    w = np.linalg.eigvalsh(C)[:, ::-1]
    ref = sc.features_reference(count, M)
    tol = 2.0 ** -40 * np.abs(trace)
    err = np.stack([np.abs(got[k] - w[:, a]) for a, k in enumerate(("l1", "l2", "l3"))], axis=1)
    gap = (w[:, 0] - w[:, 1]) >= 2.0 ** -8 * trace
    verr = np.abs(got["verticality"] - ref["verticality"])[gap & (trace > 0)]
    pos = trace > 0
    print(f"solver {what}: {len(trace)} matrices, worst eigenvalue error / trace "
          f"{(err[pos].max(1) / trace[pos]).max() if pos.any() else 0.0:.3e}, verticality compared on {len(verr)}, worst "
          f"{verr.max() if len(verr) else 0.0:.3e}")
    assert (err <= tol[:, None]).all(), what
    assert (verr <= 2.0 ** -30).all(), what
    assert (got["l1"] >= got["l2"]).all() and (got["l2"] >= got["l3"]).all()
    ok = got["l1"] > 0
    for k, num in (("linearity", got["l1"] - got["l2"]), ("planarity", got["l2"] - got["l3"]), ("scattering", got["l3"])):
        np.testing.assert_array_equal(got[k][~ok], 0.0)
        np.testing.assert_array_equal(got[k][ok], (num / np.where(ok, got["l1"], 1.0))[ok])
    return got


_SCENE_REF = {}


def _scene_ref():
    if not _SCENE_REF:
        X, wire, x0 = sc.scene()
        count, M = sc.shape_reference(X, X, sc.SCENE_RULE["radius"])
        for a in (count, M):
            a.setflags(write=False)
        _SCENE_REF["case"] = (count, M)
    return _SCENE_REF["case"]


def test_solver_on_the_scene(cuda):
    count, M = _scene_ref()
    _solver_check(count, M, cuda, "scene")


def test_solver_edge_cases(cuda):
    k = np.arange(-20, 21, dtype=np.float32)
    zero = np.zeros_like(k)
    Q = np.zeros((1, 3), dtype=np.float32)
    cases = {
        "count 0": (np.zeros(1, np.int32), np.zeros((1, 9))),
        "count 1": sc.shape_reference(np.array([[0.3, -0.2, 0.9]], dtype=np.float32), Q, 2.0),
        "collinear": sc.shape_reference(np.stack([k, k, zero], axis=1), Q + np.float32(0.5), 100.0),
        "collinear, slanted": sc.shape_reference(np.stack([k, 2 * k, 0.5 * k], axis=1), Q, 100.0),
        "vertical line": sc.shape_reference(np.stack([zero, zero, k], axis=1), Q + np.float32(3.0), 100.0),
        "plate": sc.shape_reference(np.stack(np.meshgrid(k, k, [0.0], indexing="ij"), -1).reshape(-1, 3), Q, 100.0),
    }
    count = np.concatenate([c for c, _ in cases.values()])
    M = np.vstack([m for _, m in cases.values()])
    got = _solver_check(count, M, cuda, "edge cases")
    at = {name: i for i, name in enumerate(cases)}
    _, trace = sc.covariance(count, M)
    for name in ("count 0", "count 1"):
        for key in got:
            assert abs(got[key][at[name]]) <= (0.0 if name == "count 0" else 1e-12), (name, key)
    for name in ("collinear", "collinear, slanted", "vertical line"):
        i = at[name]
        assert abs(got["l2"][i]) <= 2.0 ** -40 * trace[i] and abs(got["l3"][i]) <= 2.0 ** -40 * trace[i]
        assert got["linearity"][i] > 1.0 - 1e-9
    assert abs(got["verticality"][at["vertical line"]] - 1.0) <= 2.0 ** -30
    assert got["verticality"][at["collinear"]] <= 2.0 ** -30
    assert abs(got["verticality"][at["collinear, slanted"]] - 0.5 / np.sqrt(5.25)) <= 2.0 ** -30
    plate = at["plate"]
    assert got["scattering"][plate] <= 1e-12 and got["planarity"][plate] > 1.0 - 1e-9 and got["linearity"][plate] < 1e-9


# ------------------------------------------------------------------ g. the wire removal
def _gf(X, cuda):
    pts = _dev(X, cuda)
    return dict(points=pts, index=torch.arange(len(X), dtype=torch.int32, device=cuda), count=len(X),
                aabb=np.concatenate([X.min(0), X.max(0)]).astype(np.float32), centroid=np.zeros(3, np.float32))


def test_drop_linear_rows_on_the_scene(cuda):
    X, wire, x0 = sc.scene()
    count, M = _scene_ref()
    f = sc.features_reference(count, M)
    rule = sc.SCENE_RULE
    want = (f["linearity"] >= rule["linearity"]) & (f["verticality"] <= rule["verticality"]) & (count >= rule["min_rows"])
    near = (np.abs(f["linearity"] - rule["linearity"]) <= 1e-9) | (np.abs(f["verticality"] - rule["verticality"]) <= 1e-9)
    assert near.mean() <= 0.001
    gf = _gf(X, cuda)
    out = pipeline.drop_linear_rows(gf, **rule)
    dropped = out["dropped"].cpu().numpy()
    assert dropped.dtype == np.bool_ and dropped.shape == (len(X),)
    np.testing.assert_array_equal(dropped[~near], want[~near])
    assert out["n_dropped"] == int(dropped.sum()) and out["count"] == len(X) - out["n_dropped"]
    assert not dropped[~wire].any() and dropped[wire & (x0 > 10) & (x0 < 50)].all()
    np.testing.assert_array_equal(out["points"].cpu().numpy(), X[~dropped])   # file order
    np.testing.assert_array_equal(out["index"].cpu().numpy(), np.flatnonzero(~dropped))
    np.testing.assert_array_equal(out["aabb"], np.concatenate([X[~dropped].min(0), X[~dropped].max(0)]))
    assert gf["count"] == len(X) and gf["points"].shape[0] == len(X)          # a copy: the input is as it was
    labels, _, k = ops.dbscan(out["points"], 8.0, 20, 0, aabb=out["aabb"])
    assert k == 2 and int((labels < 0).sum()) == 0
    with pytest.raises(ValueError):
        pipeline.drop_linear_rows(dict(gf, points=gf["points"][:0], count=0), **rule)
    wide = X.copy()
    wide[0, 0] = np.float32(3.0e30)                                            # a grid beyond the 64-bit cell key
    with pytest.raises(RuntimeError, match="compressed"):
        pipeline.drop_linear_rows(_gf(wide, cuda), **rule)


def test_cluster_points_with_and_without_the_drop(cuda):
    raw = _dev(sc.scene_with_ground(), cuda)
    on = pipeline.cluster_points(raw, eps=8.0, min_points=20, chunk_size=0, drop_linear=dict(sc.SCENE_RULE))
    assert on["nclusters"] == 2 and on["ground"]["count"] == sc.SCENE_ROWS - on["drop_linear"]["n_dropped"]
    assert on["drop_linear"]["dropped"].shape == (sc.SCENE_ROWS,) and on["drop_linear"]["n_dropped"] > 1500
    assert on["labels"].shape[0] == on["ground"]["count"] and on["offsets"].shape[0] == 3
    off = pipeline.cluster_points(raw, eps=8.0, min_points=20, chunk_size=0)
    assert off["nclusters"] == 1 and "drop_linear" not in off
    none = pipeline.cluster_points(raw, eps=8.0, min_points=20, chunk_size=0, drop_linear=None)
    gf, labels, k, perm, offsets, stats = ops.tower_clusters(raw, 8.0, 20, 0)
    assert none["nclusters"] == k == 1
    assert torch.equal(none["labels"], labels) and torch.equal(none["perm"], perm)
    assert torch.equal(none["ground"]["points"].view(torch.int32), gf["points"].view(torch.int32))
    # the merge composes behind the drop
    merged = pipeline.cluster_points(raw, eps=8.0, min_points=20, chunk_size=0, drop_linear=dict(sc.SCENE_RULE),
                                     merge_threshold=6.0)
    assert merged["nclusters"] == 2 and merged["drop_linear"]["n_dropped"] == on["drop_linear"]["n_dropped"]
    # the plane rule takes the drop between its stage B and the clustering
    plane = pipeline.cluster_points(raw, eps=8.0, min_points=20, chunk_size=0, ground="plane",
                                    drop_linear=dict(sc.SCENE_RULE))
    assert plane["nclusters"] == 2 and plane["drop_linear"]["n_dropped"] > 1500


def test_drop_in_knob(cuda, tmp_path, monkeypatch):
    from pointcloudhookup_amd.utils import tower_extraction as te
    raw = sc.scene_with_ground()
    scales, offsets = np.array([0.001, 0.001, 0.001]), np.array([0.0, 0.0, 0.0])
    XYZ = np.round(raw.astype(np.float64) / scales).astype(np.int32)
    path = str(tmp_path / "corridor.las")
    las_bytes.build(path, XYZ, scales=scales, offsets=offsets)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(te, "OBB_MODE", "upright")

    def run():
        logs = []
        towers = te.extract_towers(path, log_callback=logs.append, min_points=20)
        return towers, logs

    assert te.DROP_LINEAR is None
    off, off_logs = run()
    assert "\n=== 开始杆塔检测（候选簇：1个） ===" in off_logs and len(off) == 0 and not any("剔除" in m for m in off_logs)
    monkeypatch.setattr(te, "DROP_LINEAR", te.drop_linear_from_env("2,0.9,0.5,10"))
    on, logs = run()
    extra = [m for m in logs if "剔除" in m]
    assert len(extra) == 1 and f"/{sc.SCENE_ROWS} 点" in extra[0]
    assert "\n=== 开始杆塔检测（候选簇：2个） ===" in logs and len(on) == 2
    assert sorted(round(float(t["center"][0]), -1) for t in on) == [0.0, 60.0]
    assert [m for m in logs if "剔除" not in m] != off_logs                    # two towers are reported now
    monkeypatch.setattr(te, "DROP_LINEAR", None)
    again, again_logs = run()
    assert again_logs == off_logs and len(again) == 0
