"""CPU suite: the numpy statements of tests/prims_cases.py against brute force at small sizes, and the arithmetic the
GPU cases of test_gpu_prims.py / test_gpu_segment.py rely on to reach the routes they name (no GPU, no library call)."""
import numpy as np
import pytest

import prims_cases as pc


# ------------------------------------------------------------------ statements against brute force
@pytest.mark.parametrize("n", [0, 1, 9, 300])
def test_scan_statement_is_the_running_sum(n):
    for kind in pc.SCAN_VALUES + ("wrap",):
        if kind == "wrap" and n == 0:
            continue
        v = pc.scan_values(kind, n)
        want, total = pc.scan_loop(v)
        got, got_total = pc.scan_reference(v)
        np.testing.assert_array_equal(got, want, err_msg=kind)
        assert got_total == total, kind
    big = np.array([0xFFFFFFFF, 0xFFFFFFFF, 5], dtype=np.uint32)          # the sum wraps, as uint32 arithmetic does
    np.testing.assert_array_equal(pc.scan_reference(big)[0], [0, 0xFFFFFFFF, 0xFFFFFFFE])
    assert pc.scan_reference(big)[1] == 3


def test_popcount_statement():
    words = np.concatenate([pc.scan_values(k, 500, popc=True) for k in pc.POPC_VALUES]
                           + [np.array([0, 1, 0x80000000, 0xFFFFFFFF, 0x00010001], dtype=np.uint32)])
    np.testing.assert_array_equal(pc.popcount32(words), [bin(int(w)).count("1") for w in words])
    assert pc.popcount32(np.zeros(0, np.uint32)).shape == (0,)
    # what the value kinds promise for the popcount forms
    assert set(pc.popcount32(pc.scan_values("ones", 500, popc=True))) == {1}
    assert set(pc.popcount32(pc.scan_values("small", 500, popc=True))) == {0, 1, 2, 3}
    assert pc.popcount32(pc.scan_values("spike", 5000, popc=True)).max() == 32


@pytest.mark.parametrize("nbits", [0, 1, 5, 8, 9, 17, 33, 63, 64])
@pytest.mark.parametrize("kind", pc.SORT_KEY_SETS + ("crop_fill",))
def test_sort_statement_is_a_stable_sort_of_the_low_bits(kind, nbits):
    keys, vals = pc.sort_keys(kind, 150, nbits)
    want_k, want_v = pc.insertion_sort(keys, vals, nbits)
    got_k, got_v = pc.sort_reference(keys, vals, nbits)
    np.testing.assert_array_equal(got_k, want_k)
    np.testing.assert_array_equal(got_v, want_v)
    if nbits == 0 or kind in ("high_only", "equal", "crop_fill"):        # nothing to order by: the input order stays
        np.testing.assert_array_equal(got_k, keys)
        np.testing.assert_array_equal(got_v, vals)


def test_sort_key_sets_are_what_their_names_say():
    n = 5 * pc.TILE + 77
    for nbits in (5, 13, 17, 64):
        m = pc.key_mask(nbits)
        k, v = pc.sort_keys("random", n, nbits)
        assert len(np.unique(v)) > n // 2 and not np.array_equal(v, np.arange(n))        # values are no iota
        if nbits < 64:
            assert len(np.unique(k & ~m)) > 1                                           # bits above nbits are set
        assert len(np.unique(pc.sort_keys("five", n, nbits)[0] & m)) == 5
        a = pc.sort_keys("ascending", n, nbits)[0] & m
        d = pc.sort_keys("descending", n, nbits)[0] & m
        assert np.all(a[1:] >= a[:-1]) and np.all(d[1:] <= d[:-1]) and a[0] < a[-1]
        t = pc.sort_keys("top_digit", n, nbits)[0]
        lo = 8 * (pc.sort_passes(nbits) - 1)
        assert len(np.unique(t >> np.uint64(lo))) > 1 and len(np.unique(t & pc.key_mask(lo))) == 1
        h = pc.sort_keys("high_only", n, nbits)[0]
        assert len(np.unique(h & m)) == 1 and (nbits == 64 or len(np.unique(h)) > 1)
    assert np.all(pc.sort_keys("crop_fill", 10, 13)[0] == np.uint64(0xFFFFFFFFFFFFFFFF))


@pytest.mark.parametrize("K,n", [(0, 0), (0, 50), (1, 1), (3, 0), (5, 400), (37, 3000), (300, 3000), (3000, 3000)])
def test_group_statement_is_the_mask_loop(K, n):
    xyz = pc.group_xyz(n)
    cases = [pc.group_labels(K, n)]
    if K >= 37:
        cases += [pc.group_pattern(kind, K, n) for kind in pc.GROUP_PATTERNS]
    for labels in cases:
        want = pc.group_masks(labels, xyz, K)
        got = pc.group_reference(labels, xyz, K)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and g.shape == w.shape
            np.testing.assert_array_equal(g, w)
        assert got[1].shape == (K + 1,) and got[2].shape == (K, 8)
        assert not got[2][:, 6:].any()


def test_group_patterns_are_what_their_names_say():
    n = pc.GROUP_PATTERN_N
    for K in pc.GROUP_PATTERN_K:
        lab = {kind: pc.group_pattern(kind, K, n) for kind in pc.GROUP_PATTERNS}
        assert np.all(lab["all_noise"] == -1)
        assert len(np.unique(lab["one_label"])) == 1 and 0 <= lab["one_label"][0] < K
        a = lab["alternating"]
        assert np.all(a[:-1] != a[1:]) and len(np.unique(a)) == 2 and a.min() >= 0 and a.max() < K
        r = lab["runs"]
        assert np.all(r[1:] >= r[:-1]) and r.max() < K
        for edge in (pc.TILE, 2 * pc.TILE):                  # a run ends at the edge, another crosses the next one
            assert r[edge - 1] != r[edge]
        assert r[3 * pc.TILE - 1] == r[3 * pc.TILE]
        o = lab["out_of_range"]
        for bad in (K, K + 1, pc.I32_MAX, -2, pc.I32_MIN):
            assert np.any(o == bad)
        noise = np.flatnonzero((o < 0) | (o >= K))
        perm, offsets, _ = pc.group_reference(o, pc.group_xyz(n), K)
        np.testing.assert_array_equal(perm[offsets[K]:], noise)          # among the noise rows, in row order
        size = np.diff(pc.group_reference(lab["empty_clusters"], pc.group_xyz(n), K)[1])
        empty = set(np.flatnonzero(size == 0))
        assert {0, 1, K // 2, K // 2 + 1, K - 2, K - 1} <= empty


# ------------------------------------------------------------------ what the GPU cases rely on
def test_bit_counts_and_pass_parity_of_the_grouping_sort():
    """K clusters sort on bits_for(K + 1) bits in ceil(bits / 8) passes; an odd count leaves the result in buffer 1"""
    got = {K: (pc.bits_for(K + 1), pc.sort_passes(pc.bits_for(K + 1))) for K in (255, 256, 65535, 65536)}
    assert got == {255: (8, 1), 256: (9, 2), 65535: (16, 2), 65536: (17, 3)}
    assert pc.bits_for(70001 + 1) == 17
    assert (65536, 70001) in pc.GROUP_PAIRS and (65535, 70001) in pc.GROUP_PAIRS and (255, 2049) in pc.GROUP_PAIRS
    assert [pc.sort_passes(b) & 1 for b in (0, 8, 9, 17, 64)] == [0, 1, 0, 1, 0]
    assert {pc.sort_passes(b) for b in pc.SORT_NBITS} == {0, 1, 2, 3, 4, 5, 6, 8}


def test_big_grouping_case_is_past_the_one_launch_scan():
    def table(n, K=pc.BIG_K):
        return (K + 1) * -(-n // pc.TILE)
    assert pc.BIG_K < 256 and pc.BIG_N == 10485761
    assert table(pc.BIG_N) > pc.SCAN1_LIMIT
    assert not table(pc.BIG_N - 1) > pc.SCAN1_LIMIT
    for K, n in pc.GROUP_PAIRS:                              # every other one-pass case takes the one-launch scan
        assert K >= 256 or table(max(n, 1), K) <= pc.SCAN1_LIMIT


def test_scan_sizes_reach_the_trips_and_windows_they_name():
    tiles = [-(-n // pc.TILE) for n in pc.SCAN_SIZES_CARRY]
    assert tiles == [1024, 1024, 1025, 2050]                 # 1024 tile sums per trip: one, one, two, three trips
    assert [-(-t // 1024) for t in tiles] == [1, 1, 2, 3]
    assert [-(-n // pc.TILE) for n in pc.SCAN1_SIZES[-5:]] == [256, 257, 258, 514, 642]
    assert pc.SCAN1_SIZES[-2] <= pc.SCAN1_LIMIT < pc.SCAN1_SIZES[-1]
    assert max(pc.SORT_SIZES) == 150 * pc.TILE + 3
    assert 256 * -(-max(pc.SORT_SIZES) // pc.TILE) <= 1024 * pc.TILE      # the sort's own scans stay in one trip


def test_every_scan_total_stays_below_2_31():
    """0xFFFFFFFF is the failure word of the one-launch forms, and only the "wrap" case is meant to pass 2^31"""
    for form in range(4):
        popc = form in (1, 3)
        for n, kind in pc.scan_cases(form):
            v = pc.scanned(pc.scan_values(kind, n, popc), popc)
            assert int(v.sum(dtype=np.uint64)) < 2 ** 31, (form, n, kind)
    for n in pc.TILE_SUM_SIZES:
        assert int(pc.scan_values("small", n).sum(dtype=np.uint64)) < 2 ** 31
    for n in (9, 3 * pc.TILE + 5, 1024 * pc.TILE + 1):
        assert 2 ** 31 <= int(pc.scan_values("wrap", n).sum(dtype=np.uint64)) < 2 ** 32
