"""pch_crop_boxes_f64 / ops.crop_boxes / ui.extract.crop_tower_points on the GPU against the numpy statement of
tests/crop_cases.py, bit for bit."""
import functools

import numpy as np
import pytest
import torch

import crop_cases as cc
from pointcloudhookup_amd import _lib, ops

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 2047, 2048, 2049, 70_001, 300_007]
COUNTS = [0, 1, 2, 33, 257]


@functools.lru_cache(maxsize=None)
def _cloud(n):
    return cc.cloud(n)


@functools.lru_cache(maxsize=None)
def _expected(n, T):
    return cc.expected(_cloud(n), cc.box_mix(T))


def _dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _same(got, want):
    """points, offsets, index of a call against (points, index, offsets) of the statement, bit for bit"""
    pts, offs, idx = (t.cpu().numpy() for t in got)
    assert pts.dtype == np.float64 and offs.dtype == np.int64 and idx.dtype == np.int64
    np.testing.assert_array_equal(offs, want[2])
    np.testing.assert_array_equal(idx, want[1])
    np.testing.assert_array_equal(pts.view(np.uint64), want[0].view(np.uint64))


@pytest.mark.parametrize("T", COUNTS)
@pytest.mark.parametrize("n", SIZES)
def test_crop_boxes_equals_numpy_masks(cuda, n, T):
    """for every box, points and index are the numpy mask's rows in order, offsets the cumulative counts"""
    boxes = cc.box_mix(T)
    want = _expected(n, T)
    got = ops.crop_boxes(_dev(_cloud(n), cuda), boxes, want_index=True)
    _same(got, want)
    if T >= 33 and n > 10:
        at = cc.special_positions(T)                       # the whole mix is in the case, at these places
        assert len(at) == len(cc.special_boxes()) == 23 and len(set(at)) == 23
        cnt = np.diff(want[2])[at]
        assert cnt[2] == cnt[3] and cnt[21] == cnt[22]                        # the same box twice
        assert n < 2047 or (cnt[[0, 1, 2, 9, 10, 11, 12, 13, 14, 15, 20, 21]] > 0).all()
        assert cnt[4] == 0 and cnt[5] == 0 and cnt[8] == 0                    # lo > hi; NaN bound; far outside
        assert cnt[6] == n - 1 and cnt[7] == n - 2                            # all but NaN; all but NaN and inf
        assert cnt[16] == 0 and cnt[17] == 0 and cnt[19] == 0                 # NaN in axes / centre, negative half
        assert cnt[18] == n - 2                                               # infinite half extents


def test_crop_boxes_4096_boxes(cuda):
    n, T = 70_001, 4096
    got = ops.crop_boxes(_dev(_cloud(n), cuda), cc.box_mix(T), want_index=True)
    _same(got, _expected(n, T))


def test_oriented_boxes_are_bit_equal_to_the_predicate(cuda):
    """the five named rotations with whole-metre centres and half extents (rounded rows lie exactly on the faces of
    the exact ones) and a box with a NaN in axes: empty, and it costs no other box a row"""
    n = 70_001
    P = _cloud(n)
    sp = cc.special_boxes()
    obbs = sp[11:16]
    assert all(b[0] == "obb" for b in obbs)
    for b in obbs[:3]:                                       # rows exactly ON a face exist and are taken
        d, R, h = P - b[1], np.asarray(b[2]), b[3] * 0.5
        with np.errstate(invalid="ignore"):
            u = [(d[:, 0] * R[0, k] + d[:, 1] * R[1, k]) + d[:, 2] * R[2, k] for k in range(3)]
            on = cc.inside(P, b) & ((np.abs(u[0]) == h[0]) | (np.abs(u[1]) == h[1]) | (np.abs(u[2]) == h[2]))
        assert on.sum() > 10
    want = cc.expected(P, obbs)
    assert (np.diff(want[2]) > 0).all()
    _same(ops.crop_boxes(_dev(P, cuda), obbs, want_index=True), want)
    nan_axes = sp[16]
    assert np.isnan(nan_axes[2]).any()
    with_nan = obbs[:2] + [nan_axes] + obbs[2:]
    got = ops.crop_boxes(_dev(P, cuda), with_nan, want_index=True)
    _same(got, cc.expected(P, with_nan))
    offs = got[1].cpu().numpy()
    assert offs[3] == offs[2] and offs[-1] == want[2][-1]


def test_cull_cannot_change_the_answer(cuda):
    """the same cloud in x-sorted order (tiles are thin slabs: most meet few boxes) and fully shuffled (every tile
    meets every box): per box the same set of source points"""
    n = 70_001
    Ps = cc.x_sorted(_cloud(n))
    perm = np.random.default_rng(11).permutation(n)
    Pq = Ps[perm]                                            # row j of Pq is row perm[j] of Ps
    boxes = cc.box_mix(33)
    want = cc.expected(Ps, boxes)
    gs = ops.crop_boxes(_dev(Ps, cuda), boxes, want_index=True)
    gq = ops.crop_boxes(_dev(Pq, cuda), boxes, want_index=True)
    _same(gs, want)
    _same(gq, cc.expected(Pq, boxes))
    offs, iq = gq[1].cpu().numpy(), gq[2].cpu().numpy()
    np.testing.assert_array_equal(offs, want[2])
    for t in range(len(boxes)):
        np.testing.assert_array_equal(np.sort(perm[iq[offs[t]:offs[t + 1]]]), want[1][offs[t]:offs[t + 1]])


def test_every_box_meets_every_tile(cuda):
    """257 boxes (longer than a wave's 64-box word, more than four words) that all span the full x range of an
    x-sorted cloud"""
    Ps = cc.x_sorted(_cloud(70_001))
    boxes = cc.full_x_boxes(257)
    want = cc.expected(Ps, boxes)
    assert (np.diff(want[2]) > 0).sum() > 200
    _same(ops.crop_boxes(_dev(Ps, cuda), boxes, want_index=True), want)


def test_no_tile_meets_any_box(cuda):
    Ps = cc.x_sorted(_cloud(70_001))
    boxes = cc.far_boxes(33)
    finite = np.isfinite(Ps).all(1)
    bounds = ops.crop_box_bounds(boxes)
    assert np.isfinite(bounds).all()
    lo, hi = Ps[finite].min(0), Ps[finite].max(0)
    assert not ((bounds[:, :3] <= hi).all(1) & (bounds[:, 3:] >= lo).all(1)).any()      # the premise
    pts, offs, idx = ops.crop_boxes(_dev(Ps, cuda), boxes, want_index=True)
    assert pts.shape == (0, 3) and idx.shape == (0,) and not offs.cpu().numpy().any()


@pytest.mark.parametrize("n", [2049, 300_007])
def test_one_axis_aligned_box_is_crop_aabb(cuda, n):
    """T = 1, kind 0: points, index and order are those of ops.crop_aabb on the same box"""
    (box,) = cc.box_mix(1)
    x = _dev(_cloud(n), cuda)
    pts, offs, idx = ops.crop_boxes(x, [box], want_index=True)
    ref_pts, ref_idx = ops.crop_aabb(x, box[1], box[2], want_index=True)
    assert ref_pts.shape[0] > 0
    assert torch.equal(pts.view(torch.int64), ref_pts.view(torch.int64)) and torch.equal(idx, ref_idx)
    assert offs.tolist() == [0, ref_pts.shape[0]]


def _raw_call(x, boxes, cap, room, sentinel=-12345.0):
    """the C call on buffers of `room` rows filled with a sentinel: (rc, count, offsets, points, index)"""
    L = _lib.lib()
    tab = ops.crop_box_table(boxes)
    n, T, dev = x.shape[0], len(tab), x.device
    pts = torch.full((room, 3), sentinel, dtype=torch.float64, device=dev)
    idx = torch.full((room,), -7, dtype=torch.int64, device=dev)
    offs = torch.full((T + 1,), -1, dtype=torch.int64, device=dev)
    cnt = torch.full((1,), -1, dtype=torch.int64, device=dev)
    ws = torch.empty((L.pch_crop_boxes_ws_bytes(n, T, cap) + 256,), dtype=torch.uint8, device=dev)
    rc = L.pch_crop_boxes_f64(x.data_ptr(), n, tab.ctypes.data, T, cap, pts.data_ptr(), idx.data_ptr(),
                              offs.data_ptr(), cnt.data_ptr(), ws.data_ptr(), ws.numel(),
                              torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, int(cnt.item()), offs.cpu().numpy(), pts.cpu().numpy(), idx.cpu().numpy()


@pytest.mark.parametrize("which", ["half", "zero"])
def test_cap_is_a_capacity_not_a_promise(cuda, which):
    n, T = 70_001, 33
    boxes, want = cc.box_mix(T), _expected(n, T)
    total = int(want[2][-1])
    cap = total // 2 if which == "half" else 0
    assert total > 2 * n
    x = _dev(_cloud(n), cuda)
    rc, count, offs, pts, idx = _raw_call(x, boxes, cap, room=total + 1000)
    assert rc == _lib.PCH_OK and count == total              # the true total
    np.testing.assert_array_equal(offs, want[2])             # the complete, true table
    assert (pts[cap:] == -12345.0).all() and (idx[cap:] == -7).all()          # nothing at or beyond cap
    _same(ops.crop_boxes(x, boxes, want_index=True, cap=cap), want)           # the wrapper calls once more
    # with room for everything the same call fills exactly the first `total` rows
    rc, count, offs, pts, idx = _raw_call(x, boxes, total, room=total + 1000)
    assert rc == _lib.PCH_OK and count == total
    np.testing.assert_array_equal(pts[:total].view(np.uint64), want[0].view(np.uint64))
    np.testing.assert_array_equal(idx[:total], want[1])
    assert (pts[total:] == -12345.0).all() and (idx[total:] == -7).all()


def test_c_call_limits(cuda):
    x = _dev(_cloud(2049), cuda)
    one = cc.box_mix(1)
    rc, count, offs, _, _ = _raw_call(x, [], 10, room=16)                     # no boxes: success, zeroed
    assert rc == _lib.PCH_OK and count == 0 and offs.tolist() == [0]
    rc, count, offs, _, _ = _raw_call(x[:0], one, 10, room=16)                # no rows: success, zeroed
    assert rc == _lib.PCH_OK and count == 0 and offs.tolist() == [0, 0]
    L = _lib.lib()
    tab = ops.crop_box_table(one)
    cnt = torch.zeros((1,), dtype=torch.int64, device=cuda)
    offs = torch.zeros((2,), dtype=torch.int64, device=cuda)
    out = torch.zeros((16, 3), dtype=torch.float64, device=cuda)
    ws = torch.zeros((1024,), dtype=torch.uint8, device=cuda)
    args = (x.data_ptr(), 2049, tab.ctypes.data, 1)
    tail = (out.data_ptr(), None, offs.data_ptr(), cnt.data_ptr())
    assert L.pch_crop_boxes_f64(*args, 16, *tail, ws.data_ptr(), 1024, None) == -2          # PCH_ERR_WORKSPACE
    assert L.pch_crop_boxes_f64(*args, 1 << 31, *tail, ws.data_ptr(), 1024, None) == -4     # PCH_ERR_RANGE
    assert L.pch_crop_boxes_f64(x.data_ptr(), 2049, tab.ctypes.data, 4097, 16, *tail, ws.data_ptr(), 1024, None) == -1
    tab["kind"][0] = 3
    assert L.pch_crop_boxes_f64(*args, 16, *tail, ws.data_ptr(), 1024, None) == -1          # PCH_ERR_ARG
    torch.cuda.synchronize()


def test_twice_the_same_call_gives_identical_tensors(cuda):
    n, T = 300_007, 33
    x = _dev(_cloud(n), cuda)
    a = ops.crop_boxes(x, cc.box_mix(T), want_index=True)
    b = ops.crop_boxes(x, cc.box_mix(T), want_index=True)
    assert torch.equal(a[0].view(torch.int64), b[0].view(torch.int64))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    pts, offs = ops.crop_boxes(x, cc.box_mix(T))             # without the index: the same points
    assert torch.equal(pts.view(torch.int64), a[0].view(torch.int64)) and torch.equal(offs, a[1])


# ------------------------------------------------------------------ the drop-in
@pytest.fixture(scope="module")
def tower_file(tmp_path_factory):
    """a LAS file of 40 000 points - ground, three synthetic towers - and the three tower dicts, built by hand"""
    from pointcloudhookup_amd import las
    rng = np.random.default_rng(21)
    centres = np.array([[60.0, 40.0, 18.0], [200.0, 55.0, 22.0], [330.0, 35.0, 12.0]])
    ground = rng.random((31_000, 3)) * [400.0, 100.0, 2.0]
    tw = [c + rng.normal(0.0, 1.0, (3000, 3)) * [3.0, 3.0, h / 2.5] for c, h in zip(centres, (36.0, 44.0, 18.0))]
    pts = np.vstack([ground] + tw)[rng.permutation(40_000)]
    hdr = las.LasHeader(point_format=3, version=(1, 2), scales=np.array([0.001, 0.001, 0.01]),
                        offsets=np.array([437000.0, 3139000.0, 0.0]))
    XYZ = np.round(pts / hdr.scales).astype(np.int32)
    path = str(tmp_path_factory.mktemp("crop") / "towers.las")
    las.write(path, hdr, XYZ)
    towers = [dict(center=c + hdr.offsets, rotation=cc.rot_z(20.0 * k), extent=np.array([7.0, 9.0, h]))
              for k, (c, h) in enumerate(zip(centres, (36.0, 44.0, 18.0)))]
    return path, towers


@pytest.mark.parametrize("kw", [dict(), dict(kuangxuan_preset="symmetric_moderate"),
                                dict(use_kuangxuan_method=False)], ids=["kuangxuan", "symmetric", "oriented"])
def test_crop_tower_points_equals_masks_on_the_drawn_cloud(cuda, tower_file, kw, capsys):
    from pointcloudhookup_amd.ui import extract as ex
    path, towers = tower_file
    full = ex.extract_and_visualize_towers(path, towers, **kw)[0]
    assert full.shape == (40_000, 3) and full.dtype == np.float64
    boxes = ex.tower_crop_boxes(towers, **kw)
    assert [b[0] for b in boxes] == (["obb"] * 3 if "use_kuangxuan_method" in kw else ["aabb"] * 3)
    got, rows = ex.crop_tower_points(path, towers, want_index=True, **kw)
    plain = ex.crop_tower_points(path, towers, **kw)
    assert len(got) == len(rows) == len(plain) == 3
    for b, p, r, q in zip(boxes, got, rows, plain):
        m = cc.inside(full, b)
        assert m.sum() > 2000                                # the tower is in its box
        assert r.dtype == np.int64 and p.dtype == np.float64 and p.shape == (int(m.sum()), 3)
        np.testing.assert_array_equal(r, np.flatnonzero(m))
        np.testing.assert_array_equal(p, full[m])
        np.testing.assert_array_equal(p, full[r])            # the rows index that same array
        np.testing.assert_array_equal(q, p)
    # a malformed dict: an empty array and a printed warning, the other towers unharmed
    capsys.readouterr()
    mixed = ex.crop_tower_points(path, [towers[0], dict(center=towers[1]["center"]), towers[2]], **kw)
    assert "⚠️" in capsys.readouterr().out
    assert mixed[1].shape == (0, 3)
    np.testing.assert_array_equal(mixed[0], got[0])
    np.testing.assert_array_equal(mixed[2], got[2])
