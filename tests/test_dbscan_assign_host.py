"""pch_dbscan_assign_f32 without a GPU: its all-pairs statement against real sklearn labels, the boundary cases of the
GPU tests under that statement, and the declaration of the entry points."""
import os
import re

import numpy as np
import pytest

import dbscan_assign_cases as ac
import dbscan_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FIXTURES = ["blobs600", "towers5000", "towers30000_chunk10000", "all_noise", "border_tie"]


@pytest.mark.parametrize("name", FIXTURES)
def test_own_rows_reproduce_sklearn_labels(name):
    """the rule applied to a fit's own rows gives sklearn's labels_, core rows included"""
    d = np.load(os.path.join(GOLD, f"dbscan_{name}.npz"))
    X, chunk = d["X"], int(d["chunk"])
    qc = (np.arange(len(X)) // chunk).astype(np.int32) if 0 < chunk < len(X) else None
    got = ac.assign_reference(X, d["core"], d["labels"], X, float(d["eps"]), chunk, qc, prune=len(X) > 10000)
    np.testing.assert_array_equal(got, d["labels"].astype(np.int32))
    if name == "towers30000_chunk10000":
        assert qc is not None and qc.max() == 2


def test_boundary_cases_under_the_reference():
    for name, Xf, ms, e, em, (core, lab), q in ac.boundary_cases():
        assert ac.assign_reference(Xf, core, lab, q, e).tolist() == [0], name
        assert ac.assign_reference(Xf, core, lab, q, em).tolist() == [-1], name
    Xf, ms, eps, (core, lab), inner, outer = ac.ring_case()
    assert (ac.assign_reference(Xf, core, lab, inner, eps) == 0).all()
    assert (ac.assign_reference(Xf, core, lab, outer, eps) == -1).all()


def test_reference_edge_rules():
    """sub is a float32 subtraction; bad chunks, chunk indices out of range and non-finite queries give -1; the pruned
    form states the same"""
    X = dc.bridge_cloud(12000, 31)
    rng = np.random.default_rng(3)
    core = (rng.uniform(size=len(X)) < 0.5).astype(np.uint8)
    lab = np.where(core == 1, rng.integers(0, 5, len(X)), -1).astype(np.int32)
    Q = ac.bridge_queries(X, 1.0)[::11]
    want = ac.assign_reference(X, core, lab, Q, 1.0)
    assert (want >= 0).any() and (want == -1).any()
    np.testing.assert_array_equal(ac.assign_reference(X, core, lab, Q, 1.0, prune=True), want)
    c = np.array([437000.0, 3139000.0, 80.0], dtype=np.float32)
    raw = Q + c                                                         # float32: rounds
    np.testing.assert_array_equal(ac.assign_reference(X, core, lab, raw, 1.0, sub=c),
                                  ac.assign_reference(X, core, lab, raw - c, 1.0))
    assert (ac.assign_reference(X, core, lab, Q[~np.isfinite(Q).all(1)], 1.0) == -1).all()
    qc = ac.mixed_chunks(len(Q), 3)
    got = ac.assign_reference(X, core, lab, Q, 1.0, 4000, qc)
    assert (got[(qc < 0) | (qc > 2)] == -1).all() and (got >= 0).any()
    np.testing.assert_array_equal(ac.assign_reference(X, core, lab, Q, 1.0, 4000, qc, prune=True), got)
    for k in range(3):                                                  # a chunk is its own fit
        sel = qc == k
        np.testing.assert_array_equal(got[sel], ac.assign_reference(X[4000 * k:4000 * (k + 1)], core[4000 * k:4000 * (k + 1)],
                                                                    lab[4000 * k:4000 * (k + 1)], Q[sel], 1.0))
    Xb = X.copy()
    Xb[6000, 1] = np.nan
    gb = ac.assign_reference(Xb, core, lab, Q, 1.0, 4000, qc)
    assert (gb[qc == 1] == -1).all()
    np.testing.assert_array_equal(gb[qc != 1], got[qc != 1])
    kc = ac.kept_chunks(10, [1, 2, 5, 6, 9], 2)
    assert kc.tolist() == [0, 0, 0, 1, 1, 1, 1, 2, 2, 2]


def test_entry_points_are_declared():
    from pointcloudhookup_amd import _lib
    header = open(os.path.join(ROOT, "include", "pch_hip.h")).read()
    for name in ("pch_dbscan_assign_f32", "pch_dbscan_assign_ws_bytes"):
        assert name in _lib.exported_symbols()
        assert re.search(r"\b%s\s*\(" % name, header), name
