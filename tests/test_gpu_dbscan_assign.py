"""ops.DbscanFit.assign / pch_dbscan_assign_f32: points that were not part of a fit, held against it.

Fits go through ops.DbscanFit; every expectation is dbscan_assign_cases.assign_reference, the all-pairs statement of
the rule (smallest label among the fit's core rows within eps, else -1), or a committed sklearn fixture."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import dbscan_assign_cases as ac
import dbscan_cases as dc
from pointcloudhookup_amd import _lib, ops, pipeline

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ["blobs600", "towers5000", "towers30000_chunk10000", "all_noise", "border_tie"]
EPS_C, MS_C = 1.0, 10


# ------------------------------------------------------------------ running
def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(cuda)       # a copy: cached inputs are read-only


def _fit(X, cuda, eps, ms, chunk=0, mode="auto", aabb=None):
    try:
        ops.set_dbscan_sort_mode(mode)
        return ops.DbscanFit(_dev(X, cuda), eps, ms, chunk, aabb=aabb)
    finally:
        ops.set_dbscan_sort_mode("auto")


def _assign(fit, Q, cuda, sub=None, chunk=None):
    """fit.assign on host arrays; the fit's own labels must come out of the call bit for bit as they went in"""
    before = fit.labels.clone()
    got = fit.assign(_dev(np.asarray(Q, dtype=np.float32), cuda), sub=sub,
                     chunk=None if chunk is None else _dev(np.asarray(chunk, dtype=np.int32), cuda)).cpu().numpy()
    assert torch.equal(fit.labels, before)
    return got


def _boxes(X, eps):
    """as in test_gpu_dbscan_boundary.py: the exact box, a superset that moves the grid origin, and two origins a whole
    number of cells (up to float32 rounding) below the lower corner, so that rows of the lower faces fall on cell
    faces"""
    lo, hi = X.min(0).astype(np.float64), X.max(0).astype(np.float64)
    cell = eps / math.sqrt(3.0) * (1.0 - 1.0 / 65536.0)
    out = {"exact": np.concatenate([lo, hi]),
           "superset": np.concatenate([lo - eps * np.array([0.37, 1.11, 2.73]), hi + eps * np.array([1.9, 0.2, 0.6])])}
    for name, k in (("cells-1-2-3", np.array([1.0, 2.0, 3.0])), ("cells-4-1-2", np.array([4.0, 1.0, 2.0]))):
        out[name] = np.concatenate([(lo - k * cell).astype(np.float32).astype(np.float64), hi + eps])
    return {k: v.astype(np.float32) for k, v in out.items()}


def _far(X):
    """one extra row at ~1e30: the cell key no longer fits 64 bits (compressed coordinates, or per-chunk refits)"""
    return np.vstack([X, np.array([[1e30, -1e30, 1e29]], np.float32)])


# ------------------------------------------------------------------ 1. own rows
@pytest.mark.parametrize("mode", ["chunk", "global"])
@pytest.mark.parametrize("name", FIXTURES)
def test_own_rows_give_the_sklearn_labels(cuda, name, mode):
    d = np.load(os.path.join(GOLD, f"dbscan_{name}.npz"))
    X, chunk = d["X"], int(d["chunk"])
    fit = _fit(X, cuda, float(d["eps"]), int(d["min_samples"]), chunk, mode)
    np.testing.assert_array_equal(fit.labels.cpu().numpy(), d["labels"])
    qc = (np.arange(len(X)) // chunk).astype(np.int32) if fit.chunk_size else None
    assert (qc is not None) == (name == "towers30000_chunk10000")
    got = _assign(fit, X, cuda, chunk=qc)
    np.testing.assert_array_equal(got, d["labels"].astype(np.int32))
    if name == "all_noise":
        assert fit.nclusters == 0 and (got == -1).all()


# ------------------------------------------------------------------ 2. on the boundary
def test_lone_query_at_the_boundary(cuda):
    cases = ac.boundary_cases()
    assert [c[0] for c in cases] == ["two", "one-epsg"]
    for name, Xf, ms, e, em, (core, lab), q in cases:
        for eps, want in ((e, 0), (em, -1)):
            assert ac.assign_reference(Xf, core, lab, q, eps).tolist() == [want], name
            for mode in ("chunk", "global"):
                fit = _fit(Xf, cuda, eps, ms, 0, mode)
                np.testing.assert_array_equal(fit.core.cpu().numpy(), core)
                np.testing.assert_array_equal(fit.labels.cpu().numpy(), lab)
                assert _assign(fit, q, cuda).tolist() == [want], f"{name} eps={eps!r} sort={mode}"


def test_ring_around_a_clump(cuda):
    Xf, ms, eps, (core, lab), inner, outer = ac.ring_case()
    fit = _fit(Xf, cuda, eps, ms)
    np.testing.assert_array_equal(fit.labels.cpu().numpy(), lab)
    assert len(inner) == 26 and (ac.assign_reference(Xf, core, lab, inner, eps) == 0).all()
    assert (ac.assign_reference(Xf, core, lab, outer, eps) == -1).all()
    assert (_assign(fit, inner, cuda) == 0).all()
    assert (_assign(fit, outer, cuda) == -1).all()


@pytest.mark.parametrize("name", sorted(dc.LATTICES))
def test_lattice_queries_with_pairs_exactly_at_eps(cuda, name):
    X, eps, em, mss, p = dc.lattice_case(name)
    Q = ac.lattice_queries(name)
    fit = _fit(X, cuda, eps, mss[0])
    core, lab = fit.core.cpu().numpy(), fit.labels.cpu().numpy()
    assert core[p] == 1 and fit.nclusters >= 1
    want = ac.assign_reference(X, core, lab, Q, eps)
    np.testing.assert_array_equal(want[:len(X)], lab)                  # own rows
    some = Q[::max(1, len(Q) // 2048)]
    ties = int((dc.pair_d2(X[core == 1], some) == eps * eps).sum())
    print(f"lattice {name}: {len(Q)} queries, {(want >= 0).sum()} labelled; {ties} pairs at d2 == eps*eps between "
          f"{len(some)} of them and the core rows")
    assert ties > 0
    np.testing.assert_array_equal(_assign(fit, Q, cuda), want)


# ------------------------------------------------------------------ 3. against all pairs
_BRIDGE = {}


def _bridge(cuda, chunk):
    """the bridge cloud, its queries and the reference on the fit's own core flags and labels, once per chunk size;
    the reference alone must show that the case is not empty"""
    if chunk not in _BRIDGE:
        X = dc.bridge_cloud(12000, 31)
        X.setflags(write=False)
        Q = ac.bridge_queries(X, EPS_C)
        qc = ac.mixed_chunks(len(Q), 3) if chunk else None
        fit = _fit(X, cuda, EPS_C, MS_C, chunk)
        core, lab, k = fit.core.cpu().numpy(), fit.labels.cpu().numpy(), fit.nclusters
        ref = ac.assign_reference(X, core, lab, Q, EPS_C, chunk, qc)
        labelled = np.flatnonzero(ref >= 0)
        if chunk:
            two = 0
            for c in range(3):
                s = slice(c * chunk, (c + 1) * chunk)
                sel = labelled[qc[labelled] == c]
                two += int((ac.reach_counts(X[s], core[s], lab[s], Q[sel], EPS_C) >= 2).sum())
        else:
            two = int((ac.reach_counts(X, core, lab, Q[labelled], EPS_C) >= 2).sum())
        ids = len(np.unique(ref[labelled]))
        print(f"bridge chunk={chunk}: {len(Q)} queries, {len(labelled) / len(Q):.1%} labelled, {ids} of {k} ids, "
              f"{two} queries with two clusters in reach")
        assert len(Q) == 20012 and len(labelled) >= 0.05 * len(Q) and (ref == -1).sum() >= 0.5 * len(Q)
        assert ids == k if not chunk else ids >= 50
        assert two >= 1
        for a in (Q, ref, core, lab):
            a.setflags(write=False)
        _BRIDGE[chunk] = dict(X=X, Q=Q, qc=qc, core=core, lab=lab, k=k, ref=ref)
    return _BRIDGE[chunk]


@pytest.mark.parametrize("mode", ["chunk", "global"])
@pytest.mark.parametrize("chunk", [0, 4000])
def test_bridge_queries_against_all_pairs(cuda, chunk, mode):
    b = _bridge(cuda, chunk)
    fit = _fit(b["X"], cuda, EPS_C, MS_C, chunk, mode)
    np.testing.assert_array_equal(fit.labels.cpu().numpy(), b["lab"])
    np.testing.assert_array_equal(_assign(fit, b["Q"], cuda, chunk=b["qc"]), b["ref"])
    np.testing.assert_array_equal(_assign(fit, b["Q"], cuda, chunk=b["qc"]), b["ref"])      # any number of times


@pytest.mark.parametrize("chunk", [0, 4000])
def test_many_pieces_per_cell(cuda, chunk):
    """the query set ten times over in a seeded order: 200 120 queries, many pieces per cell, several sort passes"""
    b = _bridge(cuda, chunk)
    order = np.random.default_rng(79).permutation(10 * len(b["Q"])) % len(b["Q"])
    fit = _fit(b["X"], cuda, EPS_C, MS_C, chunk)
    got = _assign(fit, b["Q"][order], cuda, chunk=None if b["qc"] is None else b["qc"][order])
    np.testing.assert_array_equal(got, b["ref"][order])


@pytest.mark.parametrize("box", ["superset", "cells-1-2-3"])
@pytest.mark.parametrize("chunk", [0, 4000])
def test_caller_supplied_box(cuda, chunk, box):
    b = _bridge(cuda, chunk)
    fit = _fit(b["X"], cuda, EPS_C, MS_C, chunk, "auto", _boxes(b["X"], EPS_C)[box])
    np.testing.assert_array_equal(fit.labels.cpu().numpy(), b["lab"])
    np.testing.assert_array_equal(_assign(fit, b["Q"], cuda, chunk=b["qc"]), b["ref"])


# ------------------------------------------------------------------ 4. sub
def test_sub_is_a_float32_subtraction(cuda):
    raw = dc.bridge_cloud(12000, 31, epsg=True)
    c = raw.astype(np.float64).mean(0).astype(np.float32)
    X = raw - c                                                        # float32, as stage B centres its rows
    eps = 16.0
    raw_q = ac.bridge_queries(raw, eps)
    raw_q = np.vstack([raw_q[:-12:4], raw_q[-12:]])                    # a quarter of them and the rows by hand
    fit = _fit(X, cuda, eps, MS_C)
    core, lab = fit.core.cpu().numpy(), fit.labels.cpu().numpy()
    want = ac.assign_reference(X, core, lab, raw_q, eps, sub=c)
    assert (want >= 0).sum() >= 0.05 * len(want) and (want == -1).sum() >= 100
    with np.errstate(invalid="ignore", over="ignore"):
        centred = raw_q - c
    assert centred.dtype == np.float32
    got = _assign(fit, raw_q, cuda, sub=c)
    np.testing.assert_array_equal(got, _assign(fit, centred, cuda))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(_assign(fit, raw, cuda, sub=c), lab)   # own rows through the subtraction


# ------------------------------------------------------------------ 5. after a relabel
def test_assign_follows_a_relabel(cuda):
    b = _bridge(cuda, 0)
    X, Q, k = b["X"], b["Q"], b["k"]
    rng = np.random.default_rng(5)
    cmap = rng.permutation(k)
    cmap[rng.choice(k, max(1, k // 3), replace=False)] = -1            # "drop a third"
    fit = _fit(X, cuda, EPS_C, MS_C)
    np.testing.assert_array_equal(_assign(fit, Q, cuda), b["ref"])     # before the relabel: the fit's own ids
    new = fit.relabel(_dev(cmap.astype(np.int32), cuda)).cpu().numpy().copy()
    np.testing.assert_array_equal(new, dc.relabel_reference(X, b["core"], b["lab"], cmap, EPS_C))
    assert ((b["lab"] >= 0) & (new == -1)).any()                        # a cluster was dropped
    np.testing.assert_array_equal(_assign(fit, X, cuda), new)          # own rows
    want = ac.assign_reference(X, b["core"], new, Q, EPS_C)
    assert (want != b["ref"]).any() and (want >= 0).any()
    np.testing.assert_array_equal(_assign(fit, Q, cuda), want)


# ------------------------------------------------------------------ 6. refusals
def test_compressed_fit_is_refused(cuda):
    X = _far(dc.bridge_cloud(6000, 32))
    fit = _fit(X, cuda, EPS_C, MS_C)
    assert fit.nclusters > 0
    before = fit.labels.clone()
    with pytest.raises(_lib.PchError, match="compressed") as err:
        fit.assign(_dev(X[:100], cuda))
    assert err.value.code == -4                                        # PCH_ERR_RANGE
    assert torch.equal(fit.labels, before)
    assert fit.first_core_rows().numel() == fit.nclusters              # the fit is still remembered


def test_per_chunk_refits_are_refused(cuda):
    X = _far(dc.bridge_cloud(6000, 32))
    fit = _fit(X, cuda, EPS_C, MS_C, 2000)
    assert fit.nclusters > 0
    qc = (np.arange(100) // 50).astype(np.int32)
    with pytest.raises(_lib.PchError, match="untouched workspace") as err:
        fit.assign(_dev(X[:100], cuda), chunk=_dev(qc, cuda))
    assert err.value.code == -1                                        # PCH_ERR_ARG


def test_a_second_fit_retires_the_first(cuda):
    X = dc.bridge_cloud(6000, 32)
    first = _fit(X, cuda, EPS_C, MS_C)
    second = _fit(X[:3000], cuda, EPS_C, MS_C)
    with pytest.raises(_lib.PchError, match="untouched workspace") as err:
        first.assign(_dev(X[:100], cuda))
    assert err.value.code == -1
    assert _assign(second, X[:100], cuda).tolist() == second.labels[:100].cpu().tolist()


def test_chunked_fit_needs_query_chunk(cuda):
    X = dc.bridge_cloud(6000, 32)
    fit = _fit(X, cuda, EPS_C, MS_C, 2000)
    assert fit.chunk_size == 2000
    with pytest.raises(_lib.PchError, match="query_chunk") as err:
        fit.assign(_dev(X[:100], cuda))
    assert err.value.code == -1
    qc = (np.arange(len(X)) // 2000).astype(np.int32)                  # refused, not forgotten
    np.testing.assert_array_equal(_assign(fit, X, cuda, chunk=qc), fit.labels.cpu().numpy())


def test_empty_queries_and_cpu_tensors(cuda):
    X = dc.bridge_cloud(6000, 32)
    fit = _fit(X, cuda, EPS_C, MS_C)
    out = fit.assign(torch.empty((0, 3), dtype=torch.float32, device=cuda))
    assert out.dtype == torch.int32 and out.numel() == 0 and out.is_cuda
    with pytest.raises(TypeError):
        fit.assign(torch.from_numpy(X[:10]))
    with pytest.raises(TypeError):
        fit.assign(_dev(X[:10], cuda), chunk=torch.zeros(10, dtype=torch.int32))


def test_query_workspace_rules(cuda):
    """the C ABI: a query workspace that is too small or overlaps the fit's is refused, and the fit stays remembered"""
    X = dc.bridge_cloud(6000, 32)
    fit = _fit(X, cuda, EPS_C, MS_C)
    L = _lib.lib()
    q = _dev(X[:500], cuda)
    out = torch.full((500,), 7, dtype=torch.int32, device=cuda)
    need = int(L.pch_dbscan_assign_ws_bytes(500))
    assert need > 0 and int(L.pch_dbscan_assign_ws_bytes(5000)) > need
    qws = torch.empty(need + 256, dtype=torch.uint8, device=cuda)
    ws = fit.workspace
    stream = torch.cuda.current_stream().cuda_stream

    def call(nq, qptr, qbytes):
        return L.pch_dbscan_assign_f32(q.data_ptr(), nq, None, None, fit.n, out.data_ptr(), qptr, qbytes, ws.data_ptr(),
                                       ws.numel(), stream)

    assert call(500, qws.data_ptr(), need - 1) == -2                   # PCH_ERR_WORKSPACE
    assert call(500, ws.data_ptr() + 4096, need) == -1                 # overlaps the fit's workspace
    assert b"overlaps" in L.pch_last_error()
    assert call(1 << 31, qws.data_ptr(), qws.numel()) == -1
    assert call(0, qws.data_ptr(), qws.numel()) == 0
    torch.cuda.synchronize()
    assert (out == 7).all()                                            # nothing was written by the refused calls
    assert call(500, qws.data_ptr(), qws.numel()) == 0                 # and the fit is still there
    np.testing.assert_array_equal(out.cpu().numpy(), fit.labels[:500].cpu().numpy())


# ------------------------------------------------------------------ 7. pipeline.label_full_cloud
_TOWERS = {}


def _towers5(cuda):
    if not _TOWERS:
        sys.path.insert(0, GOLD)
        import gen_golden as gg      # noqa: E402  (the seeded builder of refrun_towers5x3)
        x, y, z, _, _ = gg.refrun_inputs("towers5x3")
        _TOWERS["raw"] = np.stack([x, y, z], axis=1).astype(np.float32)
    return _TOWERS["raw"]


@pytest.mark.parametrize("chunk", [0, 50000])
def test_label_full_cloud(cuda, chunk):
    raw_host = _towers5(cuda)
    raw = _dev(raw_host, cuda)
    res = pipeline.label_full_cloud(raw, raw, chunk_size=chunk, segment=True)
    gf, k = res["ground"], res["nclusters"]
    index = gf["index"].cpu().numpy().astype(np.int64)
    labels, cloud = res["labels"].cpu().numpy(), res["cloud_labels"].cpu().numpy()
    assert k >= 5 and len(cloud) == len(raw_host) and len(index) > (chunk or 1)
    np.testing.assert_array_equal(cloud[index], labels)
    # the rows the filter dropped, against all pairs (pruned by cubes: the statement is the same).  The fit is made
    # again for its core flags
    pts = gf["points"].cpu().numpy()
    fit = ops.DbscanFit(gf["points"], 8.0, 80, chunk, aabb=gf["aabb"])
    np.testing.assert_array_equal(fit.labels.cpu().numpy(), labels)
    dropped = np.setdiff1d(np.arange(len(raw_host)), index)
    qc = ac.kept_chunks(len(raw_host), index, chunk) if chunk else None
    assert (qc is None) == (fit.chunk_size == 0)
    want = ac.assign_reference(pts, fit.core.cpu().numpy(), labels, raw_host[dropped], 8.0, chunk,
                               None if qc is None else qc[dropped], sub=gf["centroid"], prune=True)
    print(f"label_full_cloud chunk={chunk}: {len(index)} kept, {len(dropped)} dropped, {(want >= 0).sum()} of them labelled")
    assert (want >= 0).sum() >= 100                                    # tower feet below the threshold
    np.testing.assert_array_equal(cloud[dropped], want)
    offsets = res["offsets"].cpu().numpy()
    assert len(offsets) == k + 1 and offsets[0] == 0 and offsets[-1] == (cloud >= 0).sum()
    perm = res["perm"].cpu().numpy()[:offsets[-1]]
    assert (np.diff(offsets) > 0).all() and (cloud[perm] == np.repeat(np.arange(k), np.diff(offsets))).all()


def test_label_full_cloud_refuses_chunks_of_another_cloud(cuda):
    raw = _dev(_towers5(cuda)[:5000], cuda)
    with pytest.raises(ValueError, match="chunk_size"):
        pipeline.label_full_cloud(raw, raw.clone(), chunk_size=1000)
