"""pch_segment_by_label against the numpy statement of tests/prims_cases.py at the cluster counts, row counts and label
patterns where its routes change: one counting pass up to 255 clusters (with the one-launch or the three-launch scan
of the count table), the radix sort above, with two or three passes and the result in either ping-pong buffer.  perm,
offsets and the per-cluster boxes are compared for equality."""
import numpy as np
import pytest
import torch

import prims_cases as pc
from pointcloudhookup_amd import ops

pytestmark = pytest.mark.gpu


def _check(cuda, labels, xyz, K):
    n = len(labels)
    want_perm, want_offsets, want_stats = pc.group_reference(labels, xyz, K)
    perm, offsets, stats = ops.segment_by_label(torch.from_numpy(labels).to(cuda), torch.from_numpy(xyz).to(cuda), K)
    assert perm.dtype == torch.int32 and offsets.dtype == torch.int64 and stats.dtype == torch.float32
    assert tuple(perm.shape) == (n,) and tuple(offsets.shape) == (K + 1,) and tuple(stats.shape) == (K, 8)
    np.testing.assert_array_equal(offsets.cpu().numpy(), want_offsets)
    np.testing.assert_array_equal(perm.cpu().numpy(), want_perm)
    np.testing.assert_array_equal(stats.cpu().numpy(), want_stats)          # +inf / -inf for a cluster without rows


@pytest.mark.parametrize("K,n", pc.GROUP_PAIRS)
def test_segment_cluster_and_row_counts(cuda, K, n):
    _check(cuda, pc.group_labels(K, n), pc.group_xyz(n), K)


@pytest.mark.parametrize("K", pc.GROUP_PATTERN_K)
@pytest.mark.parametrize("kind", pc.GROUP_PATTERNS)
def test_segment_label_patterns(cuda, kind, K):
    n = pc.GROUP_PATTERN_N
    _check(cuda, pc.group_pattern(kind, K, n), pc.group_xyz(n), K)


def test_segment_one_pass_with_three_launch_scan(cuda):
    """255 clusters over 10 485 761 rows: 256 bins x 5121 tiles is the first count table past the one-launch scan"""
    K, n = pc.BIG_K, pc.BIG_N
    rng = np.random.default_rng(80)
    labels = rng.integers(-1, K, n, dtype=np.int32)
    xyz = rng.standard_normal((n, 3), dtype=np.float32)
    _check(cuda, labels, xyz, K)
