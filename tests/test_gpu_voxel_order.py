"""Opt-in canonical order of the voxel stage (pch_voxel_canonical_order, ops.voxel_downsample(order="canonical"),
import_PC.OUTPUT_ORDER): every chunk's voxels sorted by (ix, iy, iz), the order the CPU oracle emits.  All comparisons
are exact and ORDERED: neither side passes through ovx.canonical (except where a test says so)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import voxel as ovx
from pointcloudhookup_amd import las, ops, synth
from test_gpu_e2e import OFFSETS, SCALES, config1_las  # noqa: F401  (the fixture is used by name)

pytestmark = pytest.mark.gpu

OFFSET = synth.GLOBAL_OFFSET
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, cuda):
    return torch.from_numpy(np.array(a, order="C")).to(cuda)       # a copy: the shared references are read-only


def _random_case(n, voxel, chunk):
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3)) * [60.0, 25.0, 8.0] + OFFSET
    pts[: n // 3] = np.round(pts[: n // 3], 1)              # many exact duplicates / shared voxels
    return pts, voxel, chunk


def _tower_like(seed=77):
    """ground plane + a dense column, 300 000 points, two chunks (seeded: a child process builds the same rows)"""
    rng = np.random.default_rng(seed)
    g = np.column_stack([rng.uniform(0, 50, 150000), rng.uniform(0, 100, 150000), rng.normal(0, 0.05, 150000)])
    t = rng.normal([25, 50, 22], [2.5, 2.5, 9], (150000, 3))
    pts = np.vstack([g, t])
    return pts[rng.permutation(len(pts))] + OFFSET, 0.2, 200000


def _named_case(case):
    rng = np.random.default_rng(sum(case.encode()))
    if case == "all_equal_points":        # zero key bits, three chunks of one voxel each
        return np.tile(OFFSET + [1.0, 2.0, 3.0], (9000, 1)), 0.1, 4000
    if case == "huge_keys_general":       # 21+21+21 = 63 key bits plus 2 chunk bits: the two-sort route
        return rng.random((20000, 3)) * 2000.0 + OFFSET, 0.001, 6000
    if case == "wide_keys_u64":           # 18+18+14 = 50 key bits, one chunk
        return rng.random((30000, 3)) * [2000.0, 2000.0, 100.0] + OFFSET, 0.01, 0
    if case == "one_voxel_20000":         # a single voxel with 20 000 rows + scattered others
        pts = np.vstack([rng.random((20000, 3)) * 0.09 + 5.0, rng.random((3000, 3)) * 40.0]) + OFFSET
        return pts[rng.permutation(len(pts))], 0.1, 0
    if case == "dense_core":              # the finisher's paths that do not sort today
        return rng.normal(0, 0.6, (60000, 3)) + OFFSET, 0.05, 0
    assert case == "chunks_300"           # 300 chunks: the chunk-id lookup
    return rng.random((30000, 3)) * [60.0, 25.0, 8.0] + OFFSET, 0.5, 100


CASES = {"n5": lambda: _random_case(5, 0.5, 2),
         "n1000": lambda: _random_case(1000, 0.5, 300),
         "n20000": lambda: _random_case(20000, 0.2, 7000)}
CASES.update({c: (lambda c=c: _named_case(c)) for c in
              ["all_equal_points", "huge_keys_general", "wide_keys_u64", "one_voxel_20000", "dense_core",
               "chunks_300"]})
_ref_cache = {}


def _case(name):
    """(points, voxel, chunk, oracle output): computed once per session, never modified"""
    if name not in _ref_cache:
        pts, voxel, chunk = CASES[name]()
        ref = ovx.voxel_down_sample_chunked(pts, voxel, chunk if chunk else len(pts))
        for a in ref:
            a.setflags(write=False)
        _ref_cache[name] = (pts, voxel, chunk, ref)
    return _ref_cache[name]


def _equal_ordered(got, ref):
    """idx, mean (as uint64), count row by row; chunk_offsets where both sides carry them"""
    gi, gm, gc = (t.cpu().numpy() for t in got[:3])
    assert gi.shape == ref[0].shape and gm.shape == ref[1].shape and gc.shape == ref[2].shape
    np.testing.assert_array_equal(gi, ref[0])
    np.testing.assert_array_equal(gc, ref[2])
    np.testing.assert_array_equal(np.ascontiguousarray(gm).view(np.uint64), np.ascontiguousarray(ref[1]).view(np.uint64))
    if len(got) > 3:
        np.testing.assert_array_equal(got[3].cpu().numpy(), ref[3])


# ------------------------------------------------------------------------------ 5.1
@pytest.mark.parametrize("name", list(CASES))
def test_canonical_order_matches_oracle_row_by_row(cuda, name):
    pts, voxel, chunk, ref = _case(name)
    got = ops.voxel_downsample(_dev(pts, cuda), voxel, chunk, order="canonical")
    assert len(got) == 4
    _equal_ordered(got, ref)


# ------------------------------------------------------------------------------ 5.2
def _shuffled(ref, seed):
    """the rows of every chunk permuted on the host"""
    idx, mean, count, offs = ref
    rng = np.random.default_rng(seed)
    order = np.concatenate([a + rng.permutation(b - a) for a, b in zip(offs[:-1], offs[1:])]).astype(np.int64)
    return idx[order], mean[order], count[order]


@pytest.mark.parametrize("name", ["n20000", "chunks_300"])
def test_reorder_alone_restores_the_oracle_order(cuda, name):
    ref = _case(name)[3]
    sidx, smean, scount = _shuffled(ref, 5)
    assert not np.array_equal(sidx, ref[0])
    out = ops.voxel_canonical_order(_dev(sidx, cuda), _dev(smean, cuda), _dev(scount, cuda), _dev(ref[3], cuda),
                                    want_perm=True)
    assert len(out) == 4 and out[3].dtype == torch.int32
    _equal_ordered(out[:3], ref)
    perm = out[3].cpu().numpy().astype(np.int64)
    np.testing.assert_array_equal(np.sort(perm), np.arange(len(perm)))
    np.testing.assert_array_equal(sidx[perm], ref[0])
    np.testing.assert_array_equal(scount[perm], ref[2])
    np.testing.assert_array_equal(smean[perm].view(np.uint64), ref[1].view(np.uint64))
    assert len(ops.voxel_canonical_order(_dev(sidx, cuda), _dev(smean, cuda), _dev(scount, cuda),
                                         _dev(ref[3], cuda))) == 3


def test_reorder_of_indices_wider_than_one_key(cuda):
    """The call takes any non-negative int32 indices: with 31 bits on every axis the three fields alone are 93 bits, so x
    moves to the second sort beside the chunk id.  Reference: numpy's lexsort per chunk (ovx.canonical)."""
    rng = np.random.default_rng(93)
    m = 5000
    idx = rng.integers(0, 2**31, (m, 3), dtype=np.int64).astype(np.int32)
    idx[:1500, 1:] = idx[0, 1:]                                # equal (iy, iz): ordered by ix alone ...
    idx[1500:3000, :2] = idx[1500, :2]                         # ... and equal (ix, iy): ordered by iz alone
    idx[3000] = [2**31 - 1] * 3
    idx[3001] = 0
    mean = rng.random((m, 3))
    count = rng.integers(1, 100, m).astype(np.int32)
    offs = np.array([0, 1700, 1700, 4100, m], dtype=np.int64)  # an empty chunk among them
    ref = ovx.canonical(idx, mean, count, offs)
    out = ops.voxel_canonical_order(_dev(idx, cuda), _dev(mean, cuda), _dev(count, cuda), _dev(offs, cuda))
    _equal_ordered(out, ref)


def test_reorder_of_nothing_returns_empty_tensors(cuda):
    out = ops.voxel_canonical_order(torch.zeros((0, 3), dtype=torch.int32, device=cuda),
                                    torch.zeros((0, 3), dtype=torch.float64, device=cuda),
                                    torch.zeros((0,), dtype=torch.int32, device=cuda),
                                    torch.zeros((2,), dtype=torch.int64, device=cuda), want_perm=True)
    assert [tuple(t.shape) for t in out] == [(0, 3), (0, 3), (0,), (0,)]
    assert [t.dtype for t in out] == [torch.int32, torch.float64, torch.int32, torch.int32]


# ------------------------------------------------------------------------------ 5.3
def _digests(got):
    return [hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest() for t in got[:3]]


def test_canonical_order_is_the_same_on_the_finishers_other_route(cuda):
    """The stage's own order depends on its routes (PCH_VX_SCATTER is read once per process, so the other route needs a
    child); the canonical bytes must not."""
    script = r'''
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import torch
import test_gpu_voxel_order as t
pts, voxel, chunk = t._tower_like()
got = t.ops.voxel_downsample(torch.from_numpy(pts).cuda(), voxel, chunk, order="canonical")
print("digests", *t._digests(got))
'''
    env = dict(os.environ, PCH_VX_SCATTER="lds")
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "digests " in r.stdout, r.stdout[-500:] + r.stderr[-2000:]
    child = r.stdout[r.stdout.index("digests "):].split()[1:4]
    pts, voxel, chunk = _tower_like()
    got = ops.voxel_downsample(_dev(pts, cuda), voxel, chunk, order="canonical")
    assert got[3].cpu().numpy().tolist()[0] == 0 and len(got[3]) == 3
    assert _digests(got) == child


# ------------------------------------------------------------------------------ 5.4
TOWER_KEYS = ("center", "extent", "height", "width", "north_angle")


def test_dropin_canonical_output_pins_voxel_to_towers(cuda, config1_las, tmp_path, monkeypatch, capsys):
    """With OUTPUT_ORDER = "canonical" the output file is, row by row, what the host computes (scaled view -> oracle
    voxel grids -> laspy's setter), and the towers extracted from it are those of a file the test writes itself from
    the oracle's integers.  With the default order the records are the same multiset per chunk."""
    from pointcloudhookup_amd.ui import Sampling, import_PC
    from pointcloudhookup_amd.utils import tower_extraction as te
    path, XYZ, xyz, d = config1_las
    monkeypatch.chdir(tmp_path)
    ridx, rmean, rcnt, roffs = ovx.voxel_down_sample_chunked(xyz, 0.1, 500000)
    ref_XYZ = np.stack([ovx.las_unscale(rmean[:, a], SCALES[a], OFFSETS[a]) for a in range(3)], axis=1)

    monkeypatch.setattr(import_PC, "OUTPUT_ORDER", "canonical")
    out = str(tmp_path / "output" / "point_2.las")
    import_PC.run_voxel_downsampling(path, out, 0.1, 500000)
    got = las.read(out)
    np.testing.assert_array_equal(got.XYZ, ref_XYZ)                       # ordered
    towers = te.extract_towers(out, log_callback=lambda m: None)
    assert len(towers) >= 1

    mine = str(tmp_path / "oracle" / "point_2.las")
    os.makedirs(os.path.dirname(mine))
    las.write(mine, las.LasHeader(point_format=got.header.point_format, version=tuple(got.header.version),
                                  scales=SCALES, offsets=OFFSETS), ref_XYZ)
    monkeypatch.setenv("PCH_RESIDENT_HANDOFF", "0")
    want = te.extract_towers(mine, log_callback=lambda m: None)
    monkeypatch.setenv("PCH_RESIDENT_HANDOFF", "1")
    assert len(towers) == len(want)
    for t, w in zip(towers, want):
        for k in TOWER_KEYS:
            assert np.array_equal(np.asarray(t[k]), np.asarray(w[k])), k

    # the CLI twin writes the same records in the same order
    twin = str(tmp_path / "twin" / "p.las")
    Sampling.voxel_downsample_open3d(path, twin, 0.1, 500000)
    assert "成功生成下采样文件" in capsys.readouterr().out
    np.testing.assert_array_equal(las.read(twin).XYZ, ref_XYZ)
    m = Sampling.process_chunk(xyz[:20000], None, 0.5)
    np.testing.assert_array_equal(m.view(np.uint64), ovx.voxel_down_sample(xyz[:20000], 0.5)[1].view(np.uint64))

    # default order: the same multiset of records per chunk
    monkeypatch.setattr(import_PC, "OUTPUT_ORDER", "library")
    plain = str(tmp_path / "plain" / "point_2.las")
    import_PC.run_voxel_downsampling(path, plain, 0.1, 500000)
    p = las.read(plain).XYZ
    assert len(p) == len(ref_XYZ)
    for c in range(len(roffs) - 1):
        a, b = int(roffs[c]), int(roffs[c + 1])
        np.testing.assert_array_equal(p[a:b][np.lexsort(p[a:b].T[::-1])], ref_XYZ[a:b][np.lexsort(ref_XYZ[a:b].T[::-1])])

    monkeypatch.setattr(import_PC, "OUTPUT_ORDER", "sorted")
    with pytest.raises(ValueError):
        import_PC.run_voxel_downsampling(path, plain, 0.1, 500000)


# ------------------------------------------------------------------------------ 5.5
def test_interface_errors(cuda):
    x = torch.zeros((10, 3), dtype=torch.float64, device=cuda)
    with pytest.raises(ValueError):
        ops.voxel_downsample(x, 0.1, 0, order="sorted")
    with pytest.raises(TypeError, match="no CPU fallback"):
        ops.voxel_canonical_order(torch.zeros((4, 3), dtype=torch.int32), torch.zeros((4, 3), dtype=torch.float64),
                                  torch.ones((4,), dtype=torch.int32), torch.tensor([0, 4]))
    with pytest.raises(TypeError, match="no CPU fallback"):
        ops.voxel_downsample(x.cpu(), 0.1, 0, order="canonical")


@pytest.mark.parametrize("name", ["n5", "n1000", "n20000"])
def test_default_order_holds_the_same_rows(cuda, name):
    """sanity: the default call (order unspecified) is set-equal per chunk to the canonical one"""
    pts, voxel, chunk, ref = _case(name)
    idx, mean, count, offs = ops.voxel_downsample(_dev(pts, cuda), voxel, chunk)
    offs = offs.cpu().numpy()
    np.testing.assert_array_equal(offs, ref[3])
    gi, gm, gc = ovx.canonical(idx.cpu().numpy(), mean.cpu().numpy(), count.cpu().numpy(), offs)
    np.testing.assert_array_equal(gi, ref[0])
    np.testing.assert_array_equal(gc, ref[2])
    np.testing.assert_array_equal(gm.view(np.uint64), ref[1].view(np.uint64))
