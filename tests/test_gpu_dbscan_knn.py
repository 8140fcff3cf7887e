"""ops.DbscanFit.knn / pch_dbscan_knn_f32: the k nearest rows on a retained fit, and what is built on them
(ops.knn_mean_distance, pipeline.drop_sparse_rows, cluster_points(drop_sparse=...)).

Fits go through ops.DbscanFit; every expectation is knn_cases.knn_reference, the all-pairs statement of the rule, and
rows, d2 (as uint64) and count are compared bit for bit."""
import os

import numpy as np
import pytest
import torch

import dbscan_assign_cases as ac
import dbscan_cases as dc
import kdist_cases as kc
import knn_cases as kn
import las_bytes
import shape_cases as sc
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["blobs600", "towers5000", "towers30000_chunk10000", "all_noise", "border_tie"]
EPS_C, MS_C = 1.0, 10


# ------------------------------------------------------------------ running
def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(cuda)       # a copy: cached inputs are read-only


def _fit(X, cuda, eps, ms, chunk=0, mode="auto"):
    try:
        ops.set_dbscan_sort_mode(mode)
        return ops.DbscanFit(_dev(X, cuda), eps, ms, chunk)
    finally:
        ops.set_dbscan_sort_mode("auto")


def _knn(fit, Q, k, cuda, sub=None, chunk=None):
    """(rows, d2, count) of fit.knn on host arrays; the fit's labels and core flags must come out as they went in"""
    labels, core = fit.labels.clone(), fit.core.clone()
    if chunk is not None and not isinstance(chunk, str):
        chunk = _dev(np.asarray(chunk, dtype=np.int32), cuda)
    q = _dev(np.asarray(Q, dtype=np.float32), cuda)
    rows, d2, count = fit.knn(q, k, sub=sub, chunk=chunk, want_count=True)
    assert rows.dtype == torch.int32 and d2.dtype == torch.float64 and count.dtype == torch.int32
    assert rows.shape == (len(Q), k) and d2.shape == (len(Q), k) and count.shape == (len(Q),) and rows.is_cuda
    assert torch.equal(fit.labels, labels) and torch.equal(fit.core, core)
    return rows.cpu().numpy(), d2.cpu().numpy(), count.cpu().numpy()


def _same(got, want, what=""):
    """want: a reference answer of at least as many slots - its first k are the answer for k"""
    k = got[0].shape[1]
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"count {what}")
    np.testing.assert_array_equal(got[1].view(np.uint64), np.ascontiguousarray(want[1][:, :k]).view(np.uint64),
                                  err_msg=f"d2 {what}")
    np.testing.assert_array_equal(got[0], want[0][:, :k], err_msg=f"rows {what}")


def _check_ks(fit, X, Q, eps, ks, cuda, chunk_size=0, qc=None, sub=None, what=""):
    """fit.knn against the reference for every k of ks (one reference at the largest k: the answer for a smaller k is
    its first k slots); returns the reference"""
    want = kn.knn_reference(X, Q, eps, max(ks), chunk_size, qc, sub=sub)
    for k in ks:
        _same(_knn(fit, Q, k, cuda, sub=sub, chunk=qc), want, f"{what} k={k}")
    return want


# ------------------------------------------------------------------ a. own rows
_OWN = {}


def _own(name):
    if name not in _OWN:
        d = np.load(os.path.join(GOLD, f"dbscan_{name}.npz"))
        X, eps, ms, chunk = d["X"], float(d["eps"]), int(d["min_samples"]), int(d["chunk"])
        ks = sorted({1, 2, ms, min(ms + 1, ops.KNN_MAX_K)})
        qc = (np.arange(len(X)) // chunk).astype(np.int32) if 0 < chunk < len(X) else None
        want = kn.knn_reference(X, X, eps, max(ks), chunk, qc)
        for a in want:
            a.setflags(write=False)
        _OWN[name] = dict(X=X, eps=eps, ms=ms, chunk=chunk, ks=ks, want=want, core=d["core"])
    return _OWN[name]


@pytest.mark.parametrize("mode", ["chunk", "global"])
@pytest.mark.parametrize("name", FIXTURES)
def test_own_rows(cuda, name, mode):
    o = _own(name)
    X, eps, ms, want = o["X"], o["eps"], o["ms"], o["want"]
    fit = _fit(X, cuda, eps, ms, o["chunk"], mode)
    np.testing.assert_array_equal(fit.core.cpu().numpy(), o["core"])
    assert (fit.chunk_size != 0) == (name == "towers30000_chunk10000")
    for k in o["ks"]:
        rows, d2, cnt = _knn(fit, X, k, cuda, chunk="own")
        _same((rows, d2, cnt), want, f"{name} {mode} k={k}")
        kd2, kcnt = fit.kdist(_dev(X, cuda), k, chunk="own", want_count=True)
        np.testing.assert_array_equal(d2[:, k - 1].view(np.uint64), kd2.cpu().numpy().view(np.uint64))
        np.testing.assert_array_equal(cnt, kcnt.cpu().numpy())
        if k == 1:
            assert (d2 == 0.0).all() and (cnt >= 1).all()               # every row is finite here: itself or a twin
    if name == "towers30000_chunk10000":
        third = want[0][20000:]
        assert third[third >= 0].min() >= 20000 and want[0][10000:20000].max() < 20000  # global rows, per chunk
    if name == "all_noise":
        assert fit.nclusters == 0 and (want[2] < ms).all()
    if name == "border_tie":
        assert len(X) < 64
    qc = None if not fit.chunk_size else (np.arange(len(X)) // fit.chunk_size).astype(np.int32)
    _same(_knn(fit, X, ms, cuda, chunk=qc), want)                       # the explicit chunk tensor says what "own" says


# ------------------------------------------------------------------ b. lattices: ties cut by k, answers at eps*eps
@pytest.mark.parametrize("name", ["few", "tile", "dense"])
def test_lattices_with_ties_at_the_cut(cuda, name):
    X, eps, _, mss, _ = dc.lattice_case(name)
    ks = [2, 7, 27]
    want = kn.knn_reference(X, X, eps, 28)
    cut = sum(int((np.isfinite(want[1][:, k]) & (want[1][:, k - 1] == want[1][:, k])).sum()) for k in ks)
    at_eps = int((want[1][:, :27] == eps * eps).sum())
    print(f"lattice {name}: {cut} answers cut inside a tie, {at_eps} slots exactly at eps*eps")
    assert cut > 0 and (at_eps > 0 or want[2].min() > 27)
    for mode in ("chunk", "global"):
        fit = _fit(X, cuda, eps, mss[0], 0, mode)
        for k in ks:
            _same(_knn(fit, X, k, cuda), want, f"lattice {name} {mode} k={k}")
    # rows whose whole neighbourhood fits the answer end exactly at eps*eps
    kmax = int(min(want[2].max(), ops.KNN_MAX_K))
    full = kn.knn_reference(X, X, eps, kmax)
    last = full[1][np.arange(len(X)), np.minimum(full[2], kmax) - 1]
    assert (last == eps * eps).sum() > 0
    _same(_knn(fit, X, kmax, cuda), full, f"lattice {name} k={kmax}")


# ------------------------------------------------------------------ c. beyond the kept keys: re-sweeps and the row select
def test_neighbourhood_beyond_an_on_chip_buffer(cuda):
    X, rows = kc.big_cloud()
    ks = [1, 2, 64, 65, 255, 256]
    want = kn.knn_reference(X, X[rows], kc.BIG_EPS, 256)
    share = float((want[2] > 1024).mean())
    d2 = want[1]
    twins = int(((d2[:, 1:] == d2[:, :-1]) & np.isfinite(d2[:, 1:])).sum())
    cut = {k: int((np.isfinite(d2[:, k]) & (d2[:, k - 1] == d2[:, k])).sum()) for k in ks[:-1]}
    print(f"big cloud: {share:.3f} of the queries have more than 1024 rows in reach, largest count {want[2].max()}; "
          f"{twins} equal neighbours in the answers, answers cut inside a tie per k {cut}")
    assert share >= 0.6 and twins > 10000 and min(cut.values()) > 0
    fit = _fit(X, cuda, kc.BIG_EPS, 80)
    for k in ks:
        _same(_knn(fit, X[rows], k, cuda), want, f"big k={k}")


# ------------------------------------------------------------------ d. foreign queries, sub, NaN chunks, pieces
_BRIDGE = {}


def _bridge():
    if not _BRIDGE:
        X = dc.bridge_cloud(12000, 31)
        Q = ac.bridge_queries(X, EPS_C)
        Q = np.vstack([Q[:-12:3], Q[-12:]])                            # a third of them and the rows by hand
        for a in (X, Q):
            a.setflags(write=False)
        _BRIDGE.update(X=X, Q=Q)
    return _BRIDGE["X"], _BRIDGE["Q"]


@pytest.mark.parametrize("mode", ["chunk", "global"])
@pytest.mark.parametrize("chunk", [0, 4000])
def test_foreign_queries(cuda, chunk, mode):
    X, Q = _bridge()
    qc = ac.mixed_chunks(len(Q), 3) if chunk else None
    fit = _fit(X, cuda, EPS_C, MS_C, chunk, mode)
    rows, d2, cnt = _check_ks(fit, X, Q, EPS_C, [1, 3, MS_C, 30], cuda, chunk, qc, what=f"bridge chunk={chunk}")
    bad = ~np.isfinite(Q).all(1)
    s = ac.cell_side(EPS_C)
    lo, hi = X.min(0), X.max(0)
    far = ((Q < lo - 3.0 * s) | (Q > hi + 3.0 * s)).any(1) & ~bad       # more than two cells outside the grid
    assert bad.sum() == 3 and far.sum() >= 100 and (cnt[bad | far] == 0).all() and (rows[bad | far] == -1).all()
    short = (cnt > 0) & (cnt < 30)
    assert 0.1 <= (cnt > 0).mean() <= 0.9 and (cnt >= 30).mean() >= 0.002 and short.any()
    if chunk:
        out = (qc < 0) | (qc > 2)
        assert out.sum() >= 2 and (cnt[out] == 0).all() and (rows[out] == -1).all() and np.isinf(d2[out]).all()
        assert (rows[qc == 2] >= 8000).sum() > 0                        # global rows
    _same(_knn(fit, Q, 3, cuda, chunk=qc), (rows, d2, cnt))            # any number of times


def test_sub_is_a_float32_subtraction(cuda):
    raw = dc.bridge_cloud(12000, 31, epsg=True)
    c = raw.astype(np.float64).mean(0).astype(np.float32)
    X = raw - c                                                        # float32, as stage B centres its rows
    eps = 16.0
    raw_q = ac.bridge_queries(raw, eps)
    raw_q = np.vstack([raw_q[:-12:8], raw_q[-12:]])
    fit = _fit(X, cuda, eps, MS_C)
    want = _check_ks(fit, X, raw_q, eps, [1, 50], cuda, sub=c, what="sub")
    assert 0.1 <= (want[2] >= 50).mean() <= 0.95
    with np.errstate(invalid="ignore", over="ignore"):
        centred = raw_q - c
    _same(_knn(fit, centred, 50, cuda), want)
    rows, d2, n_in = _knn(fit, raw, 1, cuda, sub=c, chunk="own")        # own rows through the subtraction
    assert (d2 == 0.0).all() and (n_in >= 1).all()


def test_a_chunk_holding_nan_answers_nothing(cuda):
    X = dc.bridge_cloud(12000, 31).copy()
    X[5000, 2] = np.nan
    Q = _bridge()[1]
    qc = ac.mixed_chunks(len(Q), 3)
    fit = _fit(X, cuda, EPS_C, MS_C, 4000)
    rows, d2, cnt = _check_ks(fit, X, Q, EPS_C, [1, 5], cuda, 4000, qc, what="nan chunk")
    assert (cnt[qc == 1] == 0).all() and (rows[qc == 1] == -1).all() and (cnt[qc != 1] > 0).any()
    rows, d2, n_in = _knn(fit, X, 1, cuda, chunk="own")
    own_chunk = np.arange(len(X)) // 4000
    assert (rows[own_chunk == 1] == -1).all() and np.isinf(d2[own_chunk == 1]).all() and (d2[own_chunk != 1] == 0).all()


def test_pieces_of_one_cell(cuda):
    """65, 193 and 200 queries inside one cell each and one query 200 times over; the answers do not depend on the
    order of the queries"""
    X = _bridge()[0]
    rng = np.random.default_rng(41)
    s = ac.cell_side(EPS_C)
    o = X.min(0).astype(np.float64)
    cells = dc.grid_cells(X, EPS_C)
    uniq, cnts = np.unique(cells, axis=0, return_counts=True)
    parts = []
    for cell, m in zip(uniq[np.argsort(-cnts, kind="stable")[:3]], (65, 193, 200)):
        q = (o + (cell + 0.5) * s + rng.uniform(-0.3 * s, 0.3 * s, (m, 3))).astype(np.float32)
        assert (dc.grid_cells(q, EPS_C, origin=X.min(0)) == cell).all()
        parts.append(q)
    parts.append(np.repeat(parts[0][:1], 200, axis=0))
    Q = np.vstack(parts)
    fit = _fit(X, cuda, EPS_C, MS_C)
    ks = [1, 2, 30]
    want = _check_ks(fit, X, Q, EPS_C, ks, cuda, what="pieces")
    assert (want[2] >= 30).mean() >= 0.9 and len(np.unique(want[0][-200:], axis=0)) == 1
    order = rng.permutation(len(Q))
    for k in ks:
        _same(_knn(fit, Q[order], k, cuda), tuple(a[order] for a in want), f"shuffled k={k}")


# ------------------------------------------------------------------ continuation rules
def test_answers_do_not_follow_a_relabel_and_the_fit_is_only_read(cuda):
    X, Q = _bridge()
    fit = _fit(X, cuda, EPS_C, MS_C)
    ws = fit.workspace.clone()
    before = _knn(fit, Q, MS_C, cuda)
    assert torch.equal(fit.workspace, ws)                               # not a byte of the fit's workspace moved
    k = fit.nclusters
    rng = np.random.default_rng(5)
    cmap = rng.permutation(k)
    cmap[rng.choice(k, max(1, k // 3), replace=False)] = -1
    old = fit.labels.clone()
    fit.relabel(_dev(cmap.astype(np.int32), cuda))
    assert not torch.equal(fit.labels, old)
    _same(_knn(fit, Q, MS_C, cuda), before)
    _same(before, kn.knn_reference(X, Q, EPS_C, MS_C))


def test_refusals(cuda):
    X = dc.bridge_cloud(6000, 32)
    far = np.vstack([X, np.array([[1e30, -1e30, 1e29]], np.float32)])  # the cell key no longer fits 64 bits
    fit = _fit(far, cuda, EPS_C, MS_C)
    with pytest.raises(_lib.PchError, match="compressed") as err:
        fit.knn(_dev(X[:100], cuda), 3)
    assert err.value.code == -4                                        # PCH_ERR_RANGE
    assert fit.first_core_rows().numel() == fit.nclusters              # the fit is still remembered
    fit = _fit(far, cuda, EPS_C, MS_C, 2000)                           # per-chunk refits leave no grid
    with pytest.raises(_lib.PchError, match="untouched workspace") as err:
        fit.knn(_dev(X[:100], cuda), 3, chunk=_dev((np.arange(100) // 50).astype(np.int32), cuda))
    assert err.value.code == -1                                        # PCH_ERR_ARG
    first = _fit(X, cuda, EPS_C, MS_C)
    second = _fit(X[:3000], cuda, EPS_C, MS_C)
    with pytest.raises(_lib.PchError, match="untouched workspace") as err:
        first.knn(_dev(X[:100], cuda), 3)                              # a retired fit
    assert err.value.code == -1
    rows, d2, cnt = _knn(second, X[:100], 1, cuda)
    assert (d2 == 0.0).all()
    chunked = _fit(X, cuda, EPS_C, MS_C, 2000)
    with pytest.raises(_lib.PchError, match="query_chunk") as err:
        chunked.knn(_dev(X[:100], cuda), 3)
    assert err.value.code == -1


def test_argument_errors_and_empty_queries(cuda):
    X = dc.bridge_cloud(6000, 32)
    fit = _fit(X, cuda, EPS_C, MS_C)
    q = _dev(X[:10], cuda)
    for k in (0, 257):
        with pytest.raises(ValueError, match="k must be"):
            fit.knn(q, k)
    with pytest.raises(TypeError):
        fit.knn(torch.from_numpy(X[:10].copy()), 1)
    with pytest.raises(TypeError):
        fit.knn(q, 1, chunk=torch.zeros(10, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError, match="one chunk per query"):
        fit.knn(q, 1, chunk=torch.zeros(9, dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError, match="own"):
        fit.knn(q, 1, chunk="own")                                     # ten rows are not the fitted array
    rows, d2, cnt = fit.knn(torch.empty((0, 3), dtype=torch.float32, device=cuda), 3, want_count=True)
    assert rows.shape == (0, 3) and d2.shape == (0, 3) and cnt.numel() == 0
    two = fit.knn(q, 1)
    assert len(two) == 2 and (two[1] == 0).all() and (two[0].reshape(-1).cpu() == torch.arange(10)).all()


def test_query_workspace_rules(cuda):
    """the C ABI: k outside 1..256, a query workspace that is too small or overlaps the fit's are refused, nothing is
    written by a refused call, the fit stays remembered, out_count may be NULL"""
    X = dc.bridge_cloud(6000, 32)
    fit = _fit(X, cuda, EPS_C, MS_C)
    L = _lib.lib()
    k = 3
    q = _dev(X[:500], cuda)
    rows = torch.full((500, k), 7, dtype=torch.int32, device=cuda)
    out = torch.full((500, k), 7.0, dtype=torch.float64, device=cuda)
    cnt = torch.full((500,), 7, dtype=torch.int32, device=cuda)
    need = int(L.pch_dbscan_knn_ws_bytes(500))
    assert need > 0 and int(L.pch_dbscan_knn_ws_bytes(5000)) > need and int(L.pch_dbscan_knn_ws_bytes(-1)) == 0
    qws = torch.empty(need + 256, dtype=torch.uint8, device=cuda)
    ws = fit.workspace
    stream = torch.cuda.current_stream().cuda_stream

    def call(nq, kk, qptr, qbytes, cptr=cnt.data_ptr()):
        return L.pch_dbscan_knn_f32(q.data_ptr(), nq, None, None, kk, fit.n, rows.data_ptr(), out.data_ptr(), cptr,
                                    qptr, qbytes, ws.data_ptr(), ws.numel(), stream)

    assert call(500, k, qws.data_ptr(), need - 1) == -2                # PCH_ERR_WORKSPACE
    assert call(500, k, ws.data_ptr() + 4096, need) == -1              # overlaps the fit's workspace
    assert b"overlaps" in L.pch_last_error()
    for bad_k in (0, -2, 257, 1 << 20):
        assert call(500, bad_k, qws.data_ptr(), qws.numel()) == -1
    assert call(1 << 31, k, qws.data_ptr(), qws.numel()) == -1
    assert call(0, k, qws.data_ptr(), qws.numel()) == 0
    torch.cuda.synchronize()
    assert (rows == 7).all() and (out == 7.0).all() and (cnt == 7).all()    # nothing was written by the refused calls
    want = kn.knn_reference(X, X[:500], EPS_C, k)
    assert call(500, k, qws.data_ptr(), qws.numel()) == 0              # and the fit is still there
    _same((rows.cpu().numpy(), out.cpu().numpy(), cnt.cpu().numpy()), want)
    cnt.fill_(7)
    rows.fill_(7)
    assert call(500, k, qws.data_ptr(), qws.numel(), None) == 0        # out_count may be NULL
    torch.cuda.synchronize()
    assert (cnt == 7).all()
    np.testing.assert_array_equal(rows.cpu().numpy(), want[0])


# ------------------------------------------------------------------ e. the mean distance
def test_knn_mean_distance(cuda):
    X, _ = kn.scene_with_strays()
    worst = 0.0
    for k, eps in ((8, 2.0), (32, 2.0), (256, 8.0)):
        fit = _fit(X, cuda, eps, 1)
        rows, d2, cnt = fit.knn(_dev(X, cuda), k, chunk="own", want_count=True)
        got = ops.knn_mean_distance(d2, cnt, k)
        assert got.dtype == torch.float64 and got.shape == (len(X),) and got.is_cuda
        got = got.cpu().numpy()
        want = kn.mean_distance_reference(d2.cpu().numpy(), cnt.cpu().numpy(), k)   # the same d2: bit for bit above
        full = cnt.cpu().numpy() >= k
        assert 0.2 <= full.mean() < 1.0
        assert np.isinf(got[~full]).all() and (got[~full] > 0).all() and np.isfinite(got[full]).all()
        share = float((np.abs(got[full] - want[full]) / want[full]).max() / kn.mean_distance_bound(k))
        print(f"knn_mean_distance k={k}: largest share of the bound 2(k+4)·2^-53: {share:.4f}")
        worst = max(worst, share)
    assert worst <= 1.0


# ------------------------------------------------------------------ f. the drop of sparse rows
def _gf(X, cuda):
    pts = _dev(X, cuda)
    return dict(points=pts, index=torch.arange(len(X), dtype=torch.int32, device=cuda), count=len(X),
                aabb=np.concatenate([X.min(0), X.max(0)]).astype(np.float32), centroid=np.zeros(3, np.float32))


@pytest.mark.parametrize("rule_no", [0, 1])
def test_drop_sparse_rows_on_the_scene(cuda, rule_no):
    X, kind = kn.scene_with_strays()
    rule = kn.SPARSE_RULES[rule_no]
    ref = kn.sparse_case(rule_no)
    assert ref["margin"] >= 1e-4                                        # far beyond the bound below: equal masks
    gf = _gf(X, cuda)
    out = pipeline.drop_sparse_rows(gf, **rule)
    dropped = out["dropped"].cpu().numpy()
    assert dropped.dtype == np.bool_ and dropped.shape == (len(X),)
    np.testing.assert_array_equal(dropped, ref["dropped"])
    n_full = int((ref["count"] >= rule["k"]).sum())
    bound = kn.threshold_bound(n_full, rule["k"], rule["radius"], rule["std_ratio"])
    off = abs(out["threshold"] - ref["threshold"])
    print(f"drop_sparse_rows {rule}: threshold {out['threshold']:.6f}, {off / bound:.4f} of the bound {bound:.3g}; "
          f"dropped {int(dropped.sum())}")
    assert isinstance(out["threshold"], float) and off <= bound and bound <= 1e-6 * ref["margin"] * ref["threshold"]
    assert out["n_dropped"] == int(dropped.sum()) and out["count"] == len(X) - out["n_dropped"]
    assert not dropped[kind == 1].any() and dropped[kind == 2].sum() >= 150
    np.testing.assert_array_equal(out["points"].cpu().numpy(), X[~dropped])   # file order
    np.testing.assert_array_equal(out["index"].cpu().numpy(), np.flatnonzero(~dropped))
    np.testing.assert_array_equal(out["aabb"], np.concatenate([X[~dropped].min(0), X[~dropped].max(0)]))
    assert gf["count"] == len(X) and gf["points"].shape[0] == len(X)          # a copy: the input is as it was


def test_drop_sparse_rows_edges(cuda):
    X, _ = kn.scene_with_strays()
    gf = _gf(X, cuda)
    with pytest.raises(ValueError, match="kept no rows"):
        pipeline.drop_sparse_rows(dict(gf, points=gf["points"][:0], count=0))
    wide = X.copy()
    wide[0, 0] = np.float32(3.0e30)                                            # a grid beyond the 64-bit cell key
    with pytest.raises(RuntimeError, match="compressed"):
        pipeline.drop_sparse_rows(_gf(wide, cuda))
    # fewer than two rows with k rows in reach: only the isolated rows leave, the threshold is +inf
    lone = np.array([[0, 0, 0], [0.5, 0, 0], [0, 0.5, 0], [9, 9, 9], [20, 0, 0]], dtype=np.float32)
    out = pipeline.drop_sparse_rows(_gf(lone, cuda), k=3, radius=0.6)
    assert out["threshold"] == float("inf") and out["dropped"].cpu().tolist() == [False, True, True, True, True]
    out = pipeline.drop_sparse_rows(_gf(lone, cuda), k=1, radius=0.6)            # every row finds itself at 0.0
    assert out["n_dropped"] == 0 and out["threshold"] == 0.0


def test_cluster_points_with_and_without_the_drops(cuda):
    X, kind = kn.scene_with_strays()
    raw = _dev(kn.strays_with_ground(), cuda)
    kw = dict(eps=8.0, min_points=20, chunk_size=0, want_index=True)
    both = pipeline.cluster_points(raw, drop_sparse=dict(kn.SPARSE_RULES[0]), drop_linear=dict(sc.SCENE_RULE), **kw)
    sp, li = both["drop_sparse"], both["drop_linear"]
    assert sp["dropped"].shape == (kn.STRAY_ROWS,) and sp["dropped"].dtype == torch.bool       # over stage B's rows
    assert li["dropped"].shape == (kn.STRAY_ROWS - sp["n_dropped"],)                           # over the rows left
    assert both["ground"]["count"] == kn.STRAY_ROWS - sp["n_dropped"] - li["n_dropped"] == both["labels"].shape[0]
    assert abs(sp["threshold"] - kn.sparse_case(0)["threshold"]) <= 1e-3 and li["n_dropped"] > 1500
    k_left = kind[both["ground"]["index"].cpu().numpy()]
    lab = both["labels"].cpu().numpy()
    strays_in = int((lab[k_left == 2] >= 0).sum())
    assert both["nclusters"] == 2 and strays_in <= 5
    linear = pipeline.cluster_points(raw, drop_linear=dict(sc.SCENE_RULE), **kw)
    k_left = kind[linear["ground"]["index"].cpu().numpy()]
    strays_lin = int((linear["labels"].cpu().numpy()[k_left == 2] >= 0).sum())
    print(f"strays carrying a label: {strays_in} with both drops, {strays_lin} with drop_linear alone")
    assert strays_lin >= 50 and "drop_sparse" not in linear
    only = pipeline.cluster_points(raw, drop_sparse=dict(kn.SPARSE_RULES[0]), **kw)
    assert "drop_linear" not in only and only["drop_sparse"]["n_dropped"] == sp["n_dropped"]
    assert torch.equal(only["drop_sparse"]["dropped"], sp["dropped"])
    # off: today's call, field by field
    none = pipeline.cluster_points(raw, drop_sparse=None, **kw)
    gf, labels, k, perm, offsets, stats = ops.tower_clusters(raw, 8.0, 20, 0, want_index=True)
    assert none["nclusters"] == k and "drop_sparse" not in none and "drop_linear" not in none
    assert sorted(none) == ["ground", "labels", "nclusters", "offsets", "perm", "stats"]
    for got, want in ((none["labels"], labels), (none["perm"], perm), (none["offsets"], offsets),
                      (none["stats"], stats), (none["ground"]["index"], gf["index"]),
                      (none["ground"]["points"].view(torch.int32), gf["points"].view(torch.int32))):
        assert torch.equal(got, want) if isinstance(want, torch.Tensor) else np.array_equal(got, want)
    assert sorted(none["ground"]) == sorted(gf) and none["ground"]["count"] == gf["count"]
    for key in ("aabb", "centroid"):
        np.testing.assert_array_equal(none["ground"][key], gf[key])


def test_drop_in_knob(cuda, tmp_path, monkeypatch):
    from pointcloudhookup_amd.utils import tower_extraction as te
    _, kind = kn.scene_with_strays()
    raw = kn.strays_with_ground()
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

    assert te.DROP_SPARSE is None and te.DROP_LINEAR is None
    monkeypatch.setattr(te, "DROP_LINEAR", te.drop_linear_from_env("2,0.9,0.5,10"))
    linear, linear_logs = run()
    assert len([m for m in linear_logs if "剔除" in m]) == 1
    monkeypatch.setattr(te, "DROP_SPARSE", te.drop_sparse_from_env("8,2,2"))
    both, logs = run()
    extra = [m for m in logs if "剔除" in m]
    assert len(extra) == 2 and "稀疏点剔除" in extra[0] and f"/{kn.STRAY_ROWS} 点" in extra[0]     # the sparse rows first
    n_sparse = int(extra[0].split("剔除 ")[1].split("/")[0])
    assert 300 <= n_sparse <= 450 and f"/{kn.STRAY_ROWS - n_sparse} 点" in extra[1]
    assert "\n=== 开始杆塔检测（候选簇：2个） ===" in logs and len(both) == 2
    assert sorted(round(float(t["center"][0]), -1) for t in both) == [0.0, 60.0]
    monkeypatch.setattr(te, "DROP_SPARSE", te.drop_sparse_from_env("8,1e-30,2"))   # a failure of the step ends the run
    failed, fail_logs = run()
    assert len(failed) == 0 and any("稀疏点剔除失败" in m for m in fail_logs)
    assert not any("开始聚类处理" in m for m in fail_logs)
    monkeypatch.setattr(te, "DROP_SPARSE", None)
    again, again_logs = run()
    assert again_logs == linear_logs and len(again) == len(linear)
