"""ops.DbscanFit.kdist / pch_dbscan_kdist_f32: exact k-th neighbour distances on a retained fit.

Fits go through ops.DbscanFit; every expectation is kdist_cases.kdist_reference, the all-pairs statement of the rule,
and d2 and count are compared bit for bit."""
import math
import os

import numpy as np
import pytest
import torch

import dbscan_assign_cases as ac
import dbscan_cases as dc
import kdist_cases as kc
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["blobs600", "towers5000", "towers30000_chunk10000", "all_noise", "border_tie"]
EPS_C, MS_C = 1.0, 10
INF = float("inf")


# ------------------------------------------------------------------ running
def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(cuda)       # a copy: cached inputs are read-only


def _fit(X, cuda, eps, ms, chunk=0, mode="auto"):
    try:
        ops.set_dbscan_sort_mode(mode)
        return ops.DbscanFit(_dev(X, cuda), eps, ms, chunk)
    finally:
        ops.set_dbscan_sort_mode("auto")


def _kdist(fit, Q, k, cuda, sub=None, chunk=None):
    """(d2, count) of fit.kdist on host arrays; the fit's labels and core flags must come out as they went in"""
    labels, core = fit.labels.clone(), fit.core.clone()
    if chunk is not None and not isinstance(chunk, str):
        chunk = _dev(np.asarray(chunk, dtype=np.int32), cuda)
    d2, count = fit.kdist(_dev(np.asarray(Q, dtype=np.float32), cuda), k, sub=sub, chunk=chunk, want_count=True)
    assert d2.dtype == torch.float64 and count.dtype == torch.int32 and d2.is_cuda and count.is_cuda
    assert torch.equal(fit.labels, labels) and torch.equal(fit.core, core)
    return d2.cpu().numpy(), count.cpu().numpy()


def _same(got, want_d2, want_count, what=""):
    np.testing.assert_array_equal(got[1], want_count, err_msg=f"count {what}")
    np.testing.assert_array_equal(got[0].view(np.uint64), np.asarray(want_d2).view(np.uint64), err_msg=f"d2 {what}")


def _check_ks(fit, X, Q, eps, ks, cuda, chunk_size=0, qc=None, sub=None, what=""):
    """fit.kdist against the reference for every k of ks; returns the reference"""
    ks = list(ks)
    want, cnt = kc.kdist_reference(X, Q, eps, ks, chunk_size, qc, sub=sub)
    for a, k in enumerate(ks):
        _same(_kdist(fit, Q, k, cuda, sub=sub, chunk=qc), want[a], cnt, f"{what} k={k}")
    return want, cnt


# ------------------------------------------------------------------ a. own rows
_OWN = {}


def _own(name):
    if name not in _OWN:
        d = np.load(os.path.join(GOLD, f"dbscan_{name}.npz"))
        X, eps, ms, chunk = d["X"], float(d["eps"]), int(d["min_samples"]), int(d["chunk"])
        ks = [1, 2, ms, ms + 1]
        qc = (np.arange(len(X)) // chunk).astype(np.int32) if 0 < chunk < len(X) else None
        want, cnt = kc.kdist_reference(X, X, eps, ks, chunk, qc)
        for a in (want, cnt):
            a.setflags(write=False)
        _OWN[name] = dict(X=X, eps=eps, ms=ms, chunk=chunk, ks=ks, want=want, cnt=cnt, core=d["core"], labels=d["labels"])
    return _OWN[name]


@pytest.mark.parametrize("mode", ["chunk", "global"])
@pytest.mark.parametrize("name", FIXTURES)
def test_own_rows(cuda, name, mode):
    o = _own(name)
    X, eps, ms = o["X"], o["eps"], o["ms"]
    fit = _fit(X, cuda, eps, ms, o["chunk"], mode)
    core = fit.core.cpu().numpy()
    np.testing.assert_array_equal(core, o["core"])
    assert (fit.chunk_size != 0) == (name == "towers30000_chunk10000")
    for a, k in enumerate(o["ks"]):
        d2, cnt = _kdist(fit, X, k, cuda, chunk="own")
        _same((d2, cnt), o["want"][a], o["cnt"], f"{name} {mode} k={k}")
        np.testing.assert_array_equal(core == 1, cnt >= ms)
        if k == ms:
            np.testing.assert_array_equal(core == 1, d2 <= eps * eps)
        if k == 1:
            assert (d2 == 0.0).all() and (cnt >= 1).all()               # every row is finite here: itself
    if name == "all_noise":
        assert fit.nclusters == 0 and (o["cnt"] < ms).all()
    if name == "border_tie":
        assert len(X) < 64
    # the explicit chunk tensor says what "own" says
    qc = None if not fit.chunk_size else (np.arange(len(X)) // fit.chunk_size).astype(np.int32)
    _same(_kdist(fit, X, ms, cuda, chunk=qc), o["want"][2], o["cnt"])


# ------------------------------------------------------------------ b. the k-distance clouds
@pytest.mark.parametrize("name", sorted(dc.KDIST_CLOUDS))
def test_kdist_clouds(cuda, name):
    X = dc.KDIST_CLOUDS[name]()
    eps = 0.45 if name == "tight" else 4.0
    ks = list(dc.KDIST_MS) + [81, 300]
    want, cnt = kc.kdist_reference(X, X, eps, ks)
    share = {k: float(np.isfinite(want[a]).mean()) for a, k in enumerate(ks)}
    print(f"kdist cloud {name}: eps {eps}, finite share per k {share}, largest count {cnt.max()}")
    assert share[8] >= 0.75 and 0.2 <= share[80] <= 0.8 and share[300] == 0.0      # not a test of infinities alone
    for mode in ("chunk", "global"):
        fit = _fit(X, cuda, eps, 20, 0, mode)
        for a, k in enumerate(ks):
            _same(_kdist(fit, X, k, cuda), want[a], cnt, f"{name} {mode} k={k}")


# ------------------------------------------------------------------ c. the boundary
@pytest.mark.parametrize("name", sorted(dc.KDIST_CLOUDS))
def test_picked_rows_at_the_boundary(cuda, name):
    """eps set by a row's own k-th distance: at e the answer is that matrix entry, at em = pred(e) it is +inf"""
    X = dc.KDIST_CLOUDS[name]()
    D = dc.pair_d2(X)
    total = 0
    for ms in dc.KDIST_MS:
        picks, skipped = dc.kdist_picks(X, D, ms, npick=8)
        k = max(ms, 2)
        assert len(picks) >= 4
        for row, e, em, j in picks:
            kth = np.sort(D[row])[k - 1]
            assert kth == D[row, j] and em * em < kth <= e * e
            d2, cnt = _kdist(_fit(X, cuda, e, ms), X[row:row + 1], k, cuda)
            assert d2[0] == kth and cnt[0] >= k and cnt[0] == (D[row] <= e * e).sum(), (name, ms, row)
            d2, cnt = _kdist(_fit(X, cuda, em, ms), X[row:row + 1], k, cuda)
            assert d2[0] == INF and cnt[0] == k - 1, (name, ms, row)
            total += 1
    print(f"kdist picks {name}: {total} rows at their own boundary")


@pytest.mark.parametrize("name", ["few", "tile", "dense"])
def test_lattices_with_ties_and_pairs_exactly_at_eps(cuda, name):
    X, eps, em, mss, p = dc.lattice_case(name)
    count_p = mss[0]
    ks = sorted({1, 2, 7, 27, count_p, count_p + 1})
    fit = _fit(X, cuda, eps, count_p)
    want, cnt = _check_ks(fit, X, X, eps, ks, cuda, what=f"lattice {name}")
    at_eps = int((want == eps * eps).sum())
    tied = int((want[ks.index(2)] == want[ks.index(7)]).sum())
    print(f"lattice {name}: {at_eps} answers exactly at eps*eps, {tied} rows whose 2nd and 7th distance are equal")
    assert at_eps > 0 and tied > 0 and cnt[p] == count_p
    assert np.isfinite(want[ks.index(count_p)][p]) and want[ks.index(count_p + 1)][p] == INF
    np.testing.assert_array_equal(fit.core.cpu().numpy() == 1, cnt >= count_p)


# ------------------------------------------------------------------ d. a neighbourhood beyond any on-chip buffer
def test_neighbourhood_beyond_an_on_chip_buffer(cuda):
    X, rows = kc.big_cloud()
    want, cnt = kc.kdist_reference(X, X[rows], kc.BIG_EPS, kc.BIG_KS)
    share = float((cnt >= 5000).mean())
    print(f"big cloud: {share:.3f} of the queries have 5000 rows in reach, largest count {cnt.max()}")
    assert share >= 0.6
    fit = _fit(X, cuda, kc.BIG_EPS, 80)
    for a, k in enumerate(kc.BIG_KS):
        _same(_kdist(fit, X[rows], k, cuda), want[a], cnt, f"big k={k}")


# ------------------------------------------------------------------ e. foreign queries
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
    want, cnt = _check_ks(fit, X, Q, EPS_C, [1, 3, MS_C, 30], cuda, chunk, qc, what=f"bridge chunk={chunk}")
    bad = ~np.isfinite(Q).all(1)
    s = ac.cell_side(EPS_C)
    lo, hi = X.min(0), X.max(0)
    far = ((Q < lo - 3.0 * s) | (Q > hi + 3.0 * s)).any(1) & ~bad       # more than two cells outside the grid
    print(f"bridge chunk={chunk}: {len(Q)} queries, {np.isfinite(want[0]).mean():.1%} with a neighbour, "
          f"{np.isfinite(want[3]).mean():.1%} with 30; {bad.sum()} non-finite, {far.sum()} far outside")
    assert bad.sum() == 3 and far.sum() >= 100 and (cnt[bad | far] == 0).all()
    assert 0.1 <= np.isfinite(want[0]).mean() <= 0.9 and np.isfinite(want[2]).mean() >= 0.02
    if chunk:
        out = (qc < 0) | (qc > 2)
        assert out.sum() >= 2 and (cnt[out] == 0).all() and np.isinf(want[:, out]).all()
    _same(_kdist(fit, Q, 3, cuda, chunk=qc), want[1], cnt)            # any number of times


def test_sub_is_a_float32_subtraction(cuda):
    raw = dc.bridge_cloud(12000, 31, epsg=True)
    c = raw.astype(np.float64).mean(0).astype(np.float32)
    X = raw - c                                                        # float32, as stage B centres its rows
    eps = 16.0
    raw_q = ac.bridge_queries(raw, eps)
    raw_q = np.vstack([raw_q[:-12:8], raw_q[-12:]])
    fit = _fit(X, cuda, eps, MS_C)
    want, cnt = _check_ks(fit, X, raw_q, eps, [1, 50], cuda, sub=c, what="sub")
    assert 0.1 <= np.isfinite(want[1]).mean() <= 0.95
    with np.errstate(invalid="ignore", over="ignore"):
        centred = raw_q - c
    _same(_kdist(fit, centred, 50, cuda), want[1], cnt)
    d2, n_in = _kdist(fit, raw, 1, cuda, sub=c, chunk="own")            # own rows through the subtraction
    assert (d2 == 0.0).all() and (n_in >= 1).all()


def test_a_chunk_holding_nan_answers_nothing(cuda):
    X = dc.bridge_cloud(12000, 31).copy()
    X[5000, 2] = np.nan
    Q = _bridge()[1]
    qc = ac.mixed_chunks(len(Q), 3)
    fit = _fit(X, cuda, EPS_C, MS_C, 4000)
    want, cnt = _check_ks(fit, X, Q, EPS_C, [1, 5], cuda, 4000, qc, what="nan chunk")
    assert (cnt[qc == 1] == 0).all() and np.isinf(want[:, qc == 1]).all() and np.isfinite(want[1][qc != 1]).any()
    d2, n_in = _kdist(fit, X, 1, cuda, chunk="own")
    own_chunk = np.arange(len(X)) // 4000
    assert np.isinf(d2[own_chunk == 1]).all() and (d2[own_chunk != 1] == 0.0).all()


# ------------------------------------------------------------------ f. pieces
def test_pieces_of_one_cell(cuda):
    """65, 193 and 200 queries inside one cell each (at least nine, twenty-five and twenty-five pieces of DK_PIECE = 8) and one query
    200 times over;
    the answers do not depend on the order of the queries"""
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
    want, cnt = _check_ks(fit, X, Q, EPS_C, ks, cuda, what="pieces")
    assert np.isfinite(want[2]).mean() >= 0.9 and len(np.unique(want[1][-200:])) == 1
    order = rng.permutation(len(Q))
    for a, k in enumerate(ks):
        _same(_kdist(fit, Q[order], k, cuda), want[a][order], cnt[order], f"shuffled k={k}")


# ------------------------------------------------------------------ g. continuation rules
def test_answers_do_not_follow_a_relabel_and_the_fit_is_only_read(cuda):
    X, Q = _bridge()
    fit = _fit(X, cuda, EPS_C, MS_C)
    ws = fit.workspace.clone()
    before = _kdist(fit, Q, MS_C, cuda)
    assert torch.equal(fit.workspace, ws)                               # not a byte of the fit's workspace moved
    k = fit.nclusters
    rng = np.random.default_rng(5)
    cmap = rng.permutation(k)
    cmap[rng.choice(k, max(1, k // 3), replace=False)] = -1
    old = fit.labels.clone()
    fit.relabel(_dev(cmap.astype(np.int32), cuda))
    assert not torch.equal(fit.labels, old)
    _same(_kdist(fit, Q, MS_C, cuda), *before)
    want, cnt = kc.kdist_reference(X, Q, EPS_C, MS_C)
    _same(before, want, cnt)


def test_refusals(cuda):
    X = dc.bridge_cloud(6000, 32)
    far = np.vstack([X, np.array([[1e30, -1e30, 1e29]], np.float32)])  # the cell key no longer fits 64 bits
    fit = _fit(far, cuda, EPS_C, MS_C)
    with pytest.raises(_lib.PchError, match="compressed") as err:
        fit.kdist(_dev(X[:100], cuda), 3)
    assert err.value.code == -4                                        # PCH_ERR_RANGE
    assert fit.first_core_rows().numel() == fit.nclusters              # the fit is still remembered
    fit = _fit(far, cuda, EPS_C, MS_C, 2000)                           # per-chunk refits leave no grid
    with pytest.raises(_lib.PchError, match="untouched workspace") as err:
        fit.kdist(_dev(X[:100], cuda), 3, chunk=_dev((np.arange(100) // 50).astype(np.int32), cuda))
    assert err.value.code == -1                                        # PCH_ERR_ARG
    first = _fit(X, cuda, EPS_C, MS_C)
    second = _fit(X[:3000], cuda, EPS_C, MS_C)
    with pytest.raises(_lib.PchError, match="untouched workspace") as err:
        first.kdist(_dev(X[:100], cuda), 3)                            # a retired fit
    assert err.value.code == -1
    d2, cnt = _kdist(second, X[:100], 1, cuda)
    assert (d2 == 0.0).all()
    chunked = _fit(X, cuda, EPS_C, MS_C, 2000)
    with pytest.raises(_lib.PchError, match="query_chunk") as err:
        chunked.kdist(_dev(X[:100], cuda), 3)
    assert err.value.code == -1


def test_argument_errors_and_empty_queries(cuda):
    X = dc.bridge_cloud(6000, 32)
    fit = _fit(X, cuda, EPS_C, MS_C)
    q = _dev(X[:10], cuda)
    with pytest.raises(ValueError, match="k must be"):
        fit.kdist(q, 0)
    with pytest.raises(TypeError):
        fit.kdist(torch.from_numpy(X[:10].copy()), 1)
    with pytest.raises(TypeError):
        fit.kdist(q.double(), 1)
    with pytest.raises(TypeError):
        fit.kdist(q, 1, chunk=torch.zeros(10, dtype=torch.int32))
    with pytest.raises(TypeError):
        fit.kdist(q, 1, chunk=torch.zeros(10, dtype=torch.int64, device=cuda))
    with pytest.raises(ValueError, match="one chunk per query"):
        fit.kdist(q, 1, chunk=torch.zeros(9, dtype=torch.int32, device=cuda))
    with pytest.raises(ValueError, match="own"):
        fit.kdist(q, 1, chunk="own")                                   # ten rows are not the fitted array
    d2, cnt = fit.kdist(torch.empty((0, 3), dtype=torch.float32, device=cuda), 3, want_count=True)
    assert d2.dtype == torch.float64 and d2.numel() == 0 and cnt.dtype == torch.int32 and cnt.numel() == 0
    only = fit.kdist(q, 1)
    assert isinstance(only, torch.Tensor) and (only == 0).all()


def test_query_workspace_rules(cuda):
    """the C ABI: k < 1, a query workspace that is too small or overlaps the fit's are refused, the fit stays remembered"""
    X = dc.bridge_cloud(6000, 32)
    fit = _fit(X, cuda, EPS_C, MS_C)
    L = _lib.lib()
    q = _dev(X[:500], cuda)
    out = torch.full((500,), 7.0, dtype=torch.float64, device=cuda)
    cnt = torch.full((500,), 7, dtype=torch.int32, device=cuda)
    need = int(L.pch_dbscan_kdist_ws_bytes(500))
    assert need > 0 and int(L.pch_dbscan_kdist_ws_bytes(5000)) > need
    qws = torch.empty(need + 256, dtype=torch.uint8, device=cuda)
    ws = fit.workspace
    stream = torch.cuda.current_stream().cuda_stream

    def call(nq, k, qptr, qbytes, cptr=cnt.data_ptr()):
        return L.pch_dbscan_kdist_f32(q.data_ptr(), nq, None, None, k, fit.n, out.data_ptr(), cptr, qptr, qbytes,
                                      ws.data_ptr(), ws.numel(), stream)

    assert call(500, 3, qws.data_ptr(), need - 1) == -2                # PCH_ERR_WORKSPACE
    assert call(500, 3, ws.data_ptr() + 4096, need) == -1              # overlaps the fit's workspace
    assert b"overlaps" in L.pch_last_error()
    assert call(500, 0, qws.data_ptr(), qws.numel()) == -1             # k < 1
    assert call(500, -2, qws.data_ptr(), qws.numel()) == -1
    assert call(1 << 31, 3, qws.data_ptr(), qws.numel()) == -1
    assert call(0, 3, qws.data_ptr(), qws.numel()) == 0
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (cnt == 7).all()                     # nothing was written by the refused calls
    want, wcnt = kc.kdist_reference(X, X[:500], EPS_C, 3)
    assert call(500, 3, qws.data_ptr(), qws.numel()) == 0              # and the fit is still there
    _same((out.cpu().numpy(), cnt.cpu().numpy()), want, wcnt)
    cnt.fill_(7)
    assert call(500, 3, qws.data_ptr(), qws.numel(), None) == 0        # out_count may be NULL
    torch.cuda.synchronize()
    assert (cnt == 7).all()
    np.testing.assert_array_equal(out.cpu().numpy().view(np.uint64), want.view(np.uint64))


# ------------------------------------------------------------------ h. pipeline.kdistance_profile
def test_kdistance_profile(cuda):
    X = dc.bridge_cloud(60000, 33)
    k, eps_max, chunk, sample = 20, 1.5, 50000, 4096
    pts = _dev(X, cuda)
    prof = pipeline.kdistance_profile(pts, k=k, eps_max=eps_max, chunk_size=chunk, sample=sample, seed=3)
    rows = np.sort(np.random.default_rng(3).choice(len(X), sample, replace=False))
    np.testing.assert_array_equal(prof["rows"], rows)
    assert prof["rows"].dtype == np.int64 and (prof["k"], prof["eps_max"], prof["n"]) == (k, eps_max, len(X))
    want, cnt = kc.kdist_reference(X, X[rows], eps_max, k, chunk, (rows // chunk).astype(np.int32))
    fin = np.isfinite(want)
    print(f"profile: {fin.mean():.3f} of {sample} sampled rows have {k} rows within {eps_max}; "
          f"{(rows >= chunk).sum()} of them in the second chunk")
    assert 0.2 <= fin.mean() <= 0.95 and (rows >= chunk).sum() >= 100
    np.testing.assert_array_equal(prof["kdist"].view(np.uint64), np.sort(np.sqrt(want[fin])).view(np.uint64))
    assert prof["truncated"] == int((~fin).sum()) and prof["truncated"] + len(prof["kdist"]) == sample
    np.testing.assert_array_equal(prof["count"], cnt)
    assert prof["count"].dtype == np.int32
    assert prof["knee"] == kc.knee_reference(prof["kdist"])
    assert list(prof["quantiles"]) == [5, 25, 50, 75, 90, 95, 99]
    for qq, v in prof["quantiles"].items():
        assert v == float(np.percentile(prof["kdist"], qq))
    again = pipeline.kdistance_profile(pts, k=k, eps_max=eps_max, chunk_size=chunk, sample=sample, seed=3)
    for key in ("rows", "kdist", "count"):
        np.testing.assert_array_equal(again[key], prof[key])
    assert again["truncated"] == prof["truncated"] and again["knee"] == prof["knee"]
    fit = ops.DbscanFit(pts, eps_max, k, chunk)
    core = fit.core.cpu().numpy()[rows]
    assert pipeline.core_share(prof, eps_max) == float(core.mean())
    np.testing.assert_array_equal(core == 1, fin)
    assert pipeline.core_share(prof, 0.0) == 0.0
    with pytest.raises(ValueError):
        pipeline.core_share(prof, math.nextafter(eps_max, 2.0 * eps_max))
    whole = pipeline.kdistance_profile(pts[:3000], k=5, eps_max=eps_max, sample=200_000)
    assert len(whole["rows"]) == 3000 and (whole["rows"] == np.arange(3000)).all()     # min(sample, n) rows
