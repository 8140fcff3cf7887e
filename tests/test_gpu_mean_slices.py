"""The centroid in file-order slices (pch_mean.hip, mean_seq_launch): the summary cut into K launches over
consecutive groups of 65 536 rows, level 2 and the walk of every slice but the last on a stream of their own, the
running sums handed from slice to slice.  The result must not depend on K: everything here is compared bit for bit
with numpy (or the CPU oracle) AND with the K = 1 result, on clouds small enough for a test - slicing is forced
through ops.set_mean_slices, which real calls leave at 0 (automatic: large clouds only)."""
import functools

import numpy as np
import pytest
import torch

from oracle import ground_filter as ogf
from pointcloudhookup_amd import ops, pipeline, synth
from test_gpu_ops import _mean_cases

pytestmark = pytest.mark.gpu

KS = [2, 3, 4, 7]
ROW2 = 65536                     # rows of one level-2 row: slice boundaries are multiples of it


@pytest.fixture(autouse=True)
def _reset_slices():
    yield
    ops.set_mean_slices(0)


def _mean(raw, cuda, k):
    ops.set_mean_slices(k)
    try:
        return ops.mean_seq_f32(torch.from_numpy(raw).to(cuda)).cpu().numpy()
    finally:
        ops.set_mean_slices(0)


def _same(got, ref, msg=""):
    """as test_mean_seq_distributions compares: NaN where numpy has NaN, the same bits elsewhere"""
    nan = np.isnan(ref)
    assert (np.isnan(got) == nan).all(), msg
    np.testing.assert_array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32), err_msg=msg)


@functools.lru_cache(maxsize=None)
def _distributions():
    return dict(_mean_cases())


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """(rows, numpy's centroid): built once, read by every K"""
    rng = np.random.default_rng(20260)
    if name.startswith("uniform_"):
        n = int(name.split("_")[1])
        raw = (rng.random((n, 3)) * [1000, 100, 30] + [500000.0, 3300000.0, 80.0]).astype(np.float32)
    elif name == "ones_binade_edges":
        n = 2 ** 18 + 5          # K = 4: boundaries at rows 2^16, 2^17 and 3 * 2^16
        raw = np.ones((n, 3), np.float32)
        raw[0, 1] = 0.5          # the neighbours: the same column starting from 0.5 and from 1.5
        raw[0, 2] = 1.5
    elif name == "nan_first_and_last_slice":
        raw = (rng.random((700000, 3)) * 100).astype(np.float32)
        raw[1000, 0] = np.nan    # slice 1 of every K
        raw[690000, 1] = np.nan  # the last slice of every K
    elif name == "inf_then_minus_inf":
        raw = (rng.random((700000, 3)) * 100).astype(np.float32)
        raw[5000, 2] = np.inf    # first and last level-2 row: different slices for every K >= 2
        raw[690000, 2] = -np.inf
        raw[300000, 0] = np.inf
    elif name == "hard_stretches":
        # the cloud of test_gpu_ops.py::test_mean_seq_hard_stretches_and_ragged_end, from the same seed
        rng = np.random.default_rng(77)
        n = 3_000_017
        a = rng.normal(0, 0.05, n)
        a[1_500_000:] = np.abs(rng.normal(20, 5, n - 1_500_000))
        b = rng.normal(0, 3.0, n)
        b[700_000:1_900_000] = rng.uniform(400, 500, 1_200_000)
        b[1_900_000:] = rng.normal(-450 * 1.2e6 / (n - 1_900_000), 3.0, n - 1_900_000)
        c = rng.normal(0, 1e-3, n)
        c[:5000] = -0.0
        raw = np.column_stack([a, b, c]).astype(np.float32)
    else:
        raw = _distributions()[name]
    with np.errstate(all="ignore"):
        ref = np.mean(raw, axis=0)
    return raw, ref


SIZES = [ROW2 + 1,               # the smallest cloud with two level-2 rows, the second one holding one row
         2 * ROW2,
         3 * ROW2 + 721]         # K = 4 and 7 > rows: clamped to 4 slices of one row
PLAIN = [f"uniform_{n}" for n in SIZES] + ["zero_mean", "sign_flip_walk", "nonfinite", "leading_zeros", "halves_ties",
                                           "nan_first_and_last_slice", "inf_then_minus_inf"]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name", PLAIN)
def test_sliced_centroid_equals_numpy_and_one_slice(cuda, name, k):
    raw, ref = _cloud(name)
    one = _mean(raw, cuda, 1)
    got = _mean(raw, cuda, k)
    _same(one, ref, f"{name} K=1")
    _same(got, ref, f"{name} K={k}")
    _same(got, one, f"{name} K={k} against K=1")


def test_binade_edge_on_a_slice_boundary(cuda):
    """A column of ones: the running sum changes binade exactly at rows 2^16 and 2^17, where K = 4 cuts."""
    raw, ref = _cloud("ones_binade_edges")
    assert len(raw) // ROW2 + 1 == 5                # 5 level-2 rows -> slices of 1, 1, 1 and 2 rows
    got = _mean(raw, cuda, 4)
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
    np.testing.assert_array_equal(got.view(np.uint32), _mean(raw, cuda, 1).view(np.uint32))


def test_hard_stretches_cut_by_a_boundary(cuda):
    """K = 4 on 46 level-2 rows: boundaries at rows 720 896 (inside the zero-mean stretch of column 0 and of column 2),
    1 507 328 (just behind the end of column 0's stretch, where the blind runs are dropped again) and 2 228 224 (inside
    the stretch that walks column 1's sum back through zero) - and a ragged last slice."""
    raw, ref = _cloud("hard_stretches")
    got = _mean(raw, cuda, 4)
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
    np.testing.assert_array_equal(got.view(np.uint32), _mean(raw, cuda, 1).view(np.uint32))


@functools.lru_cache(maxsize=None)
def _corridor(n):
    raw = synth.corridor_numpy(n, seed=synth.SEED0 + 3, kind="corridor", offset=True, towers=3).astype(np.float32)
    return raw, ogf.ground_filter(raw)


def _filter(raw, cuda, k):
    ops.set_mean_slices(k)
    try:
        return ops.ground_filter(torch.from_numpy(raw).to(cuda))
    finally:
        ops.set_mean_slices(0)


@pytest.mark.parametrize("n", [200_000, 1_000_000])
def test_sliced_filter_equals_oracle_and_one_slice(cuda, n):
    raw, ref = _corridor(n)
    one = _filter(raw, cuda, 1)
    for k in KS:
        got = _filter(raw, cuda, k)
        for other, what in ((one, "K=1"), (None, "oracle")):
            cen = other["centroid"] if other else ref["centroid"]
            thr = np.float32(other["threshold"]) if other else ref["threshold"]
            cnt = other["count"] if other else len(ref["filtered"])
            pts = other["points"].cpu().numpy() if other else ref["filtered"]
            idx = other["index"].cpu().numpy() if other else np.flatnonzero(ref["keep"])
            np.testing.assert_array_equal(got["centroid"].view(np.uint32), cen.view(np.uint32), err_msg=f"K={k} {what}")
            assert np.float32(got["threshold"]).view(np.uint32) == np.float32(thr).view(np.uint32), (k, what)
            assert got["count"] == cnt, (k, what)
            np.testing.assert_array_equal(got["points"].cpu().numpy().view(np.uint32), pts.view(np.uint32),
                                          err_msg=f"K={k} {what}")
            np.testing.assert_array_equal(got["index"].cpu().numpy(), idx, err_msg=f"K={k} {what}")


def test_sliced_fused_call_equals_one_slice(cuda):
    raw, _ = _corridor(1_000_000)
    t = torch.from_numpy(raw).to(cuda)

    def run(k):
        ops.set_mean_slices(k)
        try:
            cl = pipeline.cluster_points(t, 8.0, 80, 5000)
            return [cl[key].cpu().numpy() for key in ("labels", "perm", "offsets")] + [cl["ground"]["centroid"]]
        finally:
            ops.set_mean_slices(0)

    one, got = run(1), run(4)
    assert len(one[0]) > 0 and int(one[2][-1]) > 0
    for a, b, key in zip(got, one, ("labels", "perm", "offsets", "centroid")):
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert a.tobytes() == b.tobytes(), key


def test_tiled_path_ignores_the_setting(cuda):
    """Three file-order shards chained through ops.MeanShard (pch_mean_seq_partial_f32) with K forced to 4."""
    raw, ref = _cloud("zero_mean")
    n = len(raw)
    ops.set_mean_slices(4)
    run = None
    bounds = [0, n // 3 + 5, 2 * n // 3 + 1, n]
    for i in range(3):
        shard = ops.MeanShard(torch.from_numpy(raw[bounds[i]:bounds[i + 1]]).to(cuda))
        run = shard.walk(run, total_n=n if i == 2 else 0)
    np.testing.assert_array_equal(run.cpu().numpy().view(np.uint32), ref.view(np.uint32))


def _walk_stats(raw, cuda, k):
    """the walk's statistics words of one call (tools/walk_probe.py reads them the same way): per column
    [batches, window misses, exact blocks, descents] and the exact path's [passes, serial elements, blocks]"""
    from pointcloudhookup_amd import _lib
    t = torch.from_numpy(raw).to(cuda)
    ops.set_mean_slices(k)
    try:
        ops.mean_seq_f32(t)
        torch.cuda.synchronize()
        ws = ops._workspace(_lib.lib().pch_mean_seq_f32_ws_bytes(len(raw)), t.device)
        st = ws[:128].view(torch.int32).cpu().numpy()
    finally:
        ops.set_mean_slices(0)
    return st[:12].reshape(3, 4).copy(), st[16:28].reshape(3, 4)[:, :3].copy()


def test_walk_statistics_are_totals_of_one_centroid(cuda):
    """The first slice's walk stores the statistics, later ones add.  Seven level-2 rows in seven slices: every walk
    has one row, so it makes exactly one batch (the loop ends behind the row whether it descends or not) - 7 per
    column where one launch makes between 1 and 7.  Asked twice: a walk that added to the call before would double.
    Both tallies of exactly added blocks (the walk's and the exact path's) must agree, and nothing can exceed the
    number of rows or blocks."""
    raw, _ = _cloud(f"uniform_{7 * ROW2}")
    nb2, nb = 7, 7 * 64
    one, one_x = _walk_stats(raw, cuda, 1)
    for _ in range(2):
        st, ex = _walk_stats(raw, cuda, 7)
        np.testing.assert_array_equal(st[:, 0], [7, 7, 7])
        np.testing.assert_array_equal(st[:, 2], ex[:, 2])
        assert (st[:, 3] <= nb2).all() and (st[:, 2] <= nb).all() and (st >= 0).all() and (ex >= 0).all()
    assert ((one[:, 0] >= 1) & (one[:, 0] <= nb2)).all()
    np.testing.assert_array_equal(one[:, 2], one_x[:, 2])
    # a sum that grows through the binades must be opened somewhere: the totals are not empty
    assert (st[:, 3] >= 1).all() and (one[:, 3] >= 1).all()
