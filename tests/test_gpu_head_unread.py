"""The fused call (ops.tower_clusters / pch_tower_clusters_f32) with the head of stage C planned on the device:
db_headplan_k reads stage B's kept count and box where the host used to, and db_cellscatter, db_chunksort,
db_chunkcells and db_celltab run for the largest count the caller allows for before the host has read anything.

Every case runs ops.tower_clusters and compares labels, count, points, perm, offsets and stats (as uint32) bit for bit
with ops.ground_filter + ops.dbscan + ops.segment_by_label on the same cloud, and asserts the route word
(ops.last_tower_clusters_route(): 1 = the head ran unread, 0 = the host planned stage C).

The sizing hint of ops.tower_clusters is cleared in front of every call, so nf_cap is min(n, max(n // 4, 65 536)).

Two cases are not what their one-line description in the plan of this change suggests, because stage B stands between
the input and stage C:
 * a NaN and an inf in the input's x make the centroid's x NaN (numpy's mean, which the filter restates), so EVERY kept
   row is non-finite and every chunk is noise as a whole - single bad rows in two chunks cannot reach stage C through
   the fused call;
 * a call that keeps more than nf_cap fails inside ops (PCH_ERR_WORKSPACE, route 0) and ops repeats it with nf_cap = n;
   that second library call is an ordinary one and takes route 1.  The test asserts both words.

The retained-fit query: ops.DbscanFit owns its workspace, so no ops entry continues the fused call's fit; the C entry
points do (on the workspace behind the fused call's first 256 bytes), and the last test calls one through ctypes."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import dbscan as odb
from oracle import ground_filter as ogf
from pointcloudhookup_amd import _lib, ops, synth

pytestmark = pytest.mark.gpu

EPS, MIN_PTS, CHUNK = 8.0, 80, 5000


def _base(n=120000, kind="corridor"):
    return synth.corridor_numpy(n, seed=synth.SEED0, kind=kind, offset=True, towers=3).astype(np.float32)


def _kept_rows(raw, **kw):
    """input rows the filter keeps (CPU oracle; the device filter equals it bit for bit)"""
    return np.flatnonzero(ogf.ground_filter(raw, **kw)["keep"])


def _cut_to(raw, target):
    """the cloud without its last kept rows, so that exactly `target` rows are kept (the percentile moves a little
    when rows leave, hence the loop)"""
    cur = raw
    for _ in range(10):
        keep = _kept_rows(cur)
        if len(keep) == target:
            return cur
        assert len(keep) > target
        cur = np.delete(cur, keep[-(len(keep) - target):], axis=0)
    raise AssertionError("no cut keeps the wanted count")


def _fused(raw_t, eps, min_pts, chunk, **kw):
    ops._nf_hint.clear()
    g, labels, k, perm, offsets, stats = ops.tower_clusters(raw_t, eps, min_pts, chunk, **kw)
    torch.cuda.synchronize()
    return g, labels, k, perm, offsets, stats


def _check(cuda, raw, mode, route, eps=EPS, min_pts=MIN_PTS, chunk=CHUNK, **kw):
    """fused call against the three calls; returns the fused result (ground dict, labels as numpy, k)"""
    raw_t = torch.from_numpy(np.ascontiguousarray(raw)).to(cuda)
    try:
        ops.set_dbscan_sort_mode(mode)
        g, labels, k, perm, offsets, stats = _fused(raw_t, eps, min_pts, chunk, **kw)
        got_route = ops.last_tower_clusters_route()
        ref = ops.ground_filter(raw_t, want_index=False, **kw)
        assert g["count"] == ref["count"] and g["used_fallback"] == ref["used_fallback"]
        assert torch.equal(g["points"].view(torch.int32), ref["points"].view(torch.int32))
        nf = ref["count"]
        print(f"kept {nf}, clusters {k}, route {got_route}")
        if nf == 0:
            assert labels.numel() == 0 and k == 0 and offsets.cpu().tolist() == [0]
        else:
            rl, _, rk = ops.dbscan(ref["points"], eps, min_pts, chunk)
            rperm, roffsets, rstats = ops.segment_by_label(rl, ref["points"], rk)
            assert k == rk
            assert torch.equal(labels, rl)
            assert torch.equal(perm, rperm) and torch.equal(offsets, roffsets[:rk + 1])
            assert torch.equal(stats.view(torch.int32), rstats[:rk].view(torch.int32))
    finally:
        ops.set_dbscan_sort_mode("auto")
    assert got_route == route
    return g, labels.cpu().numpy(), k


# ------------------------------------------------------------------------------------------------ route 1
def test_base_cloud_runs_unread(cuda):
    raw = _base()
    g, labels, k = _check(cuda, raw, "chunk", 1)
    assert g["count"] == 11772 and k > 0
    try:
        fit = "c"
        odb._clib()
    except Exception:
        fit = "sklearn"
    want = odb.dbscan_chunked(ogf.ground_filter(raw)["filtered"], EPS, MIN_PTS, CHUNK, fit=fit)
    np.testing.assert_array_equal(labels, want)


def test_auto_mode_with_enough_chunks(cuda):
    """11 772 kept rows in chunks of 120: 99 chunks, the automatic choice is the chunk route"""
    g, _, _ = _check(cuda, _base(), "auto", 1, min_pts=10, chunk=120)
    assert -(-g["count"] // 120) >= 96


@pytest.mark.parametrize("kept", [2 * CHUNK, 2 * CHUNK + 1])
def test_kept_count_at_a_chunk_boundary(cuda, kept):
    g, _, k = _check(cuda, _cut_to(_base(), kept), "chunk", 1)
    assert g["count"] == kept and k > 0


def test_small_cloud_swept_by_gf_compact(cuda):
    """40 000 rows: below the 65 536 rows from which the summary emits candidate slots"""
    g, _, _ = _check(cuda, _base(40000), "chunk", 1, chunk=1000)
    assert g["count"] == 3926


def test_workspace_reused_larger_then_smaller(cuda):
    """the second call finds the first call's DbHead (and its longer chunk tables) in the same workspace"""
    big, small = _base(), _base(40000)
    g1, _, _ = _check(cuda, big, "chunk", 1, chunk=1000)
    g2, _, _ = _check(cuda, small, "chunk", 1, chunk=1000)
    assert g1["count"] - g2["count"] > 1000
    _check(cuda, big, "chunk", 1, chunk=1000)


def test_chunk_with_more_cells_than_the_table(cuda):
    """the kept rows of the second chunk spread over 2 km x 2 km (cells of 4.6 m): more than 1 024 cells, the chunk
    goes through the gated db_chunksort and db_celltab fills keys; x and y do not enter the filter's rule"""
    raw = _base()
    keep = _kept_rows(raw)
    rows = keep[CHUNK:2 * CHUNK]
    rng = np.random.default_rng(7)
    raw[rows, 0] += rng.uniform(0.0, 2000.0, len(rows)).astype(np.float32)
    raw[rows, 1] += rng.uniform(0.0, 2000.0, len(rows)).astype(np.float32)
    assert np.array_equal(_kept_rows(raw), keep)
    raw_t = torch.from_numpy(raw).to(cuda)
    _check(cuda, raw, "chunk", 1)
    try:                                                   # which kernels ran
        ops.set_dbscan_sort_mode("chunk")
        ops.set_profiling(True)
        _fused(raw_t, EPS, MIN_PTS, CHUNK)
        ran = {name for name, _, launches in ops.get_profile() if launches > 0}
    finally:
        ops.set_profiling(False)
        ops.set_dbscan_sort_mode("auto")
    assert {"db_headplan", "db_cellscatter", "db_chunksort", "db_chunkcells", "db_celltab", "db_heads", "db_cells"} <= ran


def test_nan_and_inf_rows(cuda):
    """see the module's docstring: every kept row is non-finite, every chunk is noise as a whole"""
    raw = _base()
    keep = _kept_rows(raw)
    raw[keep[100], 0] = np.nan
    raw[keep[CHUNK + 100], 0] = np.inf
    g, labels, k = _check(cuda, raw, "chunk", 1)
    assert g["count"] == len(keep) and k == 0 and (labels == -1).all()


# ------------------------------------------------------------------------------------------------ route 0
def test_fallback_threshold(cuda):
    g, _, _ = _check(cuda, _base(), "chunk", 0, min_keep=20000)
    assert g["used_fallback"] and g["count"] == 11866


def test_more_kept_than_the_first_call_allows(cuda):
    """78 016 of 120 000 rows kept, nf_cap 65 536: the first library call stands down and fails, the repeat is an
    ordinary call (module docstring)"""
    raw = _base(kind="uniform")
    calls = []
    real = _lib.lib().pch_tower_clusters_f32
    info_at = 17                                            # position of info_host among the arguments

    def spy(*args):
        rc = real(*args)
        info = C.cast(C.c_void_p(args[info_at]), C.POINTER(_lib.TowerClustersInfo)).contents
        calls.append((rc, int(info.reserved)))
        return rc

    L = _lib.lib()
    try:
        L.pch_tower_clusters_f32 = spy
        g, _, _ = _check(cuda, raw, "chunk", 1)
    finally:
        L.pch_tower_clusters_f32 = real
    assert g["count"] == 78016
    assert calls == [(-2, 0), (0, 1)]


def test_nothing_kept(cuda):
    raw = _base()
    raw[:, 2] = np.float32(85.0)
    g, _, _ = _check(cuda, raw, "chunk", 0)
    assert g["count"] == 0


def test_auto_mode_with_few_chunks(cuda):
    """3 chunks of 5 000: nothing is queued unread (14 chunks at nf_cap); 24 chunks of 500: the head is queued (132
    chunks at nf_cap) and stands down on the device"""
    _check(cuda, _base(), "auto", 0)
    _check(cuda, _base(), "auto", 0, chunk=500)


def test_chunk_size_above_the_chunk_sort_limit(cuda):
    """195 176 kept rows in chunks of 140 000 (the chunk sort takes 131 072): the global sort, on both library calls"""
    g, _, _ = _check(cuda, _base(300000, kind="uniform"), "chunk", 0, chunk=140000)
    assert g["count"] == 195176


def test_cell_key_beyond_31_bits(cuda):
    """one kept row 1e8 m away in x: 25 + 3 + 4 key bits per cell, the staged lists hold 31"""
    raw = _base()
    keep = _kept_rows(raw)
    raw[keep[7000], 0] += np.float32(1.0e8)
    assert np.array_equal(_kept_rows(raw), keep)
    _check(cuda, raw, "chunk", 0)


def test_key_beyond_64_bits_refits_every_chunk(cuda):
    """one kept row 1e10 m away: more than 2e9 cells along x, every chunk is fitted on its own box"""
    raw = _base()
    keep = _kept_rows(raw)
    raw[keep[7000], 0] = np.float32(1.0e10)
    assert np.array_equal(_kept_rows(raw), keep)
    _, _, k = _check(cuda, raw, "chunk", 0)
    assert k > 0


# ------------------------------------------------------------------------------------------------ the retained fit
def test_query_on_the_fused_calls_workspace(cuda):
    """pch_dbscan_first_core_rows_i32 continues the fused call's fit: stage C's part of the workspace starts behind
    the first 256 bytes and was carved for nf_cap rows, not for the kept count.  Without the grouping stage, which
    carves the same workspace and retires the fit"""
    raw_t = torch.from_numpy(_base()).to(cuda)
    try:
        ops.set_dbscan_sort_mode("chunk")
        g, labels, k, _, _, _ = _fused(raw_t, EPS, MIN_PTS, CHUNK, segment=False)
        assert ops.last_tower_clusters_route() == 1 and k > 0
        ws = ops._workspace(1, raw_t.device)                # the buffer the call used (grow-only, per thread)
        out = torch.full((k,), -7, dtype=torch.int32, device=cuda)
        with torch.cuda.device(raw_t.device):
            _lib.check(_lib.lib().pch_dbscan_first_core_rows_i32(g["count"], out.data_ptr(), ws.data_ptr() + 256,
                                                                 ws.numel() - 256, ops._stream()))
        torch.cuda.synchronize()
        fit = ops.DbscanFit(g["points"], EPS, MIN_PTS, CHUNK)
        assert torch.equal(out, fit.first_core_rows())
    finally:
        ops.set_dbscan_sort_mode("auto")
