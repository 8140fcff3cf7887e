"""Scan, radix sort and label grouping: the numpy statement of each, the brute-force forms the CPU test holds them
against, and the inputs the GPU tests use (TEST INFRASTRUCTURE, pure numpy; imported by the CPU and the GPU tests, not a
conftest).  Nothing here knows about tiles, waves or look-back; the size lists name the edges they were chosen for."""
import numpy as np

TILE = 2048                                      # elements per workgroup of the scans, the sort and the grouping
SCAN1_LIMIT = 2 ** 20 + 2 ** 18                  # largest table the one-launch scan is chosen for (scan1_pays)
GUARD = 64                                       # guard words on each side of every output
GUARD_WORD = 0xA5A5A5A5


# ------------------------------------------------------------------ the statements
def popcount32(words):
    """bits set in every uint32 word"""
    b = np.ascontiguousarray(words, dtype=np.uint32).view(np.uint8)
    return _BYTE_BITS[b].reshape(-1, 4).sum(axis=1, dtype=np.uint32)


_BYTE_BITS = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def scan_reference(v):
    """(exclusive prefix sums modulo 2^32 as uint32 [n], total modulo 2^32)"""
    v = np.asarray(v, dtype=np.uint32)
    c = np.cumsum(v, dtype=np.uint64)
    total = int(c[-1]) if len(v) else 0
    return (c - v).astype(np.uint32), total & 0xFFFFFFFF


def key_mask(nbits):
    return np.uint64((1 << nbits) - 1)


def sort_reference(keys, vals, nbits):
    """(keys[order], vals[order]) for the stable order of the low nbits key bits; the full keys travel"""
    keys = np.asarray(keys, dtype=np.uint64)
    order = np.argsort(keys & key_mask(nbits), kind="stable")
    return keys[order], np.asarray(vals, dtype=np.uint32)[order]


def bits_for(count):
    """bits needed to store values in [0, count) (pch_common.h)"""
    b = 0
    while b < 64 and (1 << b) < count:
        b += 1
    return b


def sort_passes(nbits):
    return 0 if nbits <= 0 else (nbits + 7) // 8


def bin_of(labels, K):
    labels = np.asarray(labels, dtype=np.int32).astype(np.int64)
    return np.where((labels < 0) | (labels >= K), K, labels)


def group_reference(labels, xyz, K):
    """(perm int32 [n], offsets int64 [K+1], stats float32 [K,8]) as include/pch_hip.h states pch_segment_by_label"""
    b = bin_of(labels, K)
    b = b.astype(np.uint8 if K < 256 else np.uint16 if K < 65536 else np.int64)    # narrow keys: numpy sorts by radix
    perm = np.argsort(b, kind="stable")
    offsets = np.searchsorted(b[perm], np.arange(K + 2))[:K + 1].astype(np.int64)
    stats = np.zeros((K, 8), dtype=np.float32)
    stats[:, :3], stats[:, 3:6] = np.inf, -np.inf
    size = np.diff(offsets)
    full = np.flatnonzero(size > 0)
    if len(full):
        P = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)[perm[:offsets[K]]]
        stats[full, :3] = np.minimum.reduceat(P, offsets[full], axis=0)      # starts of the non-empty clusters: each
        stats[full, 3:6] = np.maximum.reduceat(P, offsets[full], axis=0)     # segment runs to the next start
    return perm.astype(np.int32), offsets, stats


# ------------------------------------------------------------------ brute force, for the CPU test
def scan_loop(v):
    out, s = [], 0
    for x in v:
        out.append(s & 0xFFFFFFFF)
        s += int(x)
    return np.array(out, dtype=np.uint32), s & 0xFFFFFFFF


def insertion_sort(keys, vals, nbits):
    m = (1 << nbits) - 1
    rows = []
    for k, v in zip((int(k) for k in keys), (int(v) for v in vals)):
        at = len(rows)
        while at > 0 and (rows[at - 1][0] & m) > (k & m):
            at -= 1
        rows.insert(at, (k, v))
    return np.array([r[0] for r in rows], dtype=np.uint64), np.array([r[1] for r in rows], dtype=np.uint32)


def group_masks(labels, xyz, K):
    """the K-mask loop of the reference (and of test_segment_by_label)"""
    labels = np.asarray(labels, dtype=np.int32)
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    rows = [np.flatnonzero(labels == k) for k in range(K)]
    noise = np.flatnonzero((labels < 0) | (labels >= K))
    perm = np.concatenate(rows + [noise]).astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    stats = np.zeros((K, 8), dtype=np.float32)
    for k, r in enumerate(rows):
        stats[k, :3] = xyz[r].min(0) if len(r) else np.inf
        stats[k, 3:6] = xyz[r].max(0) if len(r) else -np.inf
    return perm, offsets, stats


# ------------------------------------------------------------------ scan inputs
SCAN_SIZES_SMALL = [0, 1, 7, 8, 9,                           # vector / scalar access edge (8 words per thread)
                    2047, 2048, 2049,                        # tile edge
                    3 * TILE + 5]                            # several tiles
SCAN_SIZES_CARRY = [1024 * TILE - 1, 1024 * TILE, 1024 * TILE + 1,    # the tile-sum scan's second trip: from 1025 tiles
                    2049 * TILE + 1]                                  # third trip
SCAN3_SIZES = SCAN_SIZES_SMALL + SCAN_SIZES_CARRY
# one-launch forms: the look-back fetches 256 tiles per round trip; 641 tiles is the first size past SCAN1_LIMIT
SCAN1_SIZES = SCAN_SIZES_SMALL + [t * TILE + 3 for t in (255, 256, 257, 513, 641)]
TILE_SUM_SIZES = [1, 1023, 1024, 1025, 2048, 2049, 3000]

SCAN_VALUES = ("ones", "zeros", "small", "spike")
POPC_VALUES = ("ones", "zeros", "small", "spike", "words", "runs")


_KIND_SEED = {"ones": 1, "zeros": 2, "small": 3, "spike": 4, "words": 5, "runs": 6, "wrap": 7}


def scan_values(kind, n, popc=False):
    """uint32 [n] input words.  For the popcount forms the scanned value is the bit count of each word, so "ones" is a
    word with one bit, "small" a word with 0..3 bits and "spike" one full word.  Every total stays below 2^31 except
    "wrap" (plain form only), whose total lies in [2^31, 2^32)."""
    rng = np.random.default_rng([_KIND_SEED[kind], n, int(popc)])
    if kind == "zeros":
        return np.zeros(n, dtype=np.uint32)
    if kind == "ones":
        return (np.uint32(1) << rng.integers(0, 32, n).astype(np.uint32)) if popc else np.ones(n, dtype=np.uint32)
    if kind == "small":
        c = rng.integers(0, 4, n)
        if not popc:
            return c.astype(np.uint32)
        return (np.array([0, 0x80000000, 0x00010001, 0x40000102], dtype=np.uint32))[c]
    if kind == "spike":                          # one large value at a tile's last element (or the array's)
        v = np.zeros(n, dtype=np.uint32)
        if n:
            at = min(n - 1, ((n // 2) // TILE) * TILE + TILE - 1)
            v[at] = 0xFFFFFFFF if popc else 0x7FFFFFF0      # every element behind it reads this value
        return v
    if kind == "words":
        return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "runs":                           # random words with runs of 0 and of 0xFFFFFFFF
        v = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        for s in range(0, n, 97):
            v[s:s + 40] = 0 if (s // 97) % 2 else 0xFFFFFFFF
        return v
    if kind == "wrap":                           # total in [2^31, 2^32): n values that add up to 3 * 2^30 + a bit
        assert n > 0 and not popc
        v = np.full(n, (3 << 30) // n, dtype=np.uint32)
        v[rng.integers(0, n)] += 12345
        return v
    raise ValueError(kind)


def scan_cases(form):
    """[(n, kind)] of one scan form: every size with every value kind"""
    popc = form in (1, 3)
    sizes = SCAN3_SIZES if form in (0, 1) else SCAN1_SIZES
    return [(n, k) for n in sizes for k in (POPC_VALUES if popc else SCAN_VALUES)]


def scanned(v, popc):
    return popcount32(v) if popc else np.asarray(v, dtype=np.uint32)


# ------------------------------------------------------------------ sort inputs
SORT_NBITS = [0, 1, 5, 8, 9, 16, 17, 24, 31, 32, 33, 40, 41, 63, 64]
SORT_NBITS_AT = [513, 5 * TILE + 77]
SORT_SIZES = [0, 1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 150 * TILE + 3]
SORT_SIZES_AT = [17, 64]
SORT_KEY_SETS = ("random", "five", "equal", "ascending", "descending", "top_digit", "high_only")


def sort_keys(kind, n, nbits):
    """(keys uint64 [n], vals uint32 [n]): the values are random, never an iota"""
    rng = np.random.default_rng([SORT_KEY_SETS.index(kind) if kind in SORT_KEY_SETS else 99, n, nbits])
    vals = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    full = rng.integers(0, 2 ** 64, n, dtype=np.uint64)           # random in all 64 bits: the bits above nbits too
    m = key_mask(nbits)
    if kind == "random":
        keys = full
    elif kind == "five":                         # five distinct sort keys, random bits above: stability shows in vals
        w = min(nbits, 16)                       # drawn without repeats from the top w of the nbits bits, plus low bits
        five = rng.choice(1 << w, size=min(5, 1 << w), replace=False).astype(np.uint64) << np.uint64(nbits - w)
        if nbits - w >= 9:
            five |= np.uint64(0x155)
        keys = (full & ~m) | five[rng.integers(0, len(five), n)]
    elif kind == "equal":
        keys = np.full(n, 0x0123456789ABCDEF, dtype=np.uint64)
    elif kind == "ascending":
        keys = np.sort(full & m) | (full & ~m)
    elif kind == "descending":
        keys = np.sort(full & m)[::-1] | (full & ~m)
    elif kind == "top_digit":                    # keys that differ only in the digit of the last pass
        lo = 8 * (sort_passes(nbits) - 1) if nbits > 0 else 0
        digit = np.uint64(((1 << nbits) - 1) >> lo << lo)
        keys = (full & digit) | (np.uint64(0x5A5A5A5A5A5A5A5A) & ~digit)
    elif kind == "high_only":                    # keys that differ only above nbits: the result is the input order
        keys = (full & ~m) | (np.uint64(0x0F0F0F0F0F0F0F0F) & m)
    elif kind == "crop_fill":                    # the crop's fill: every byte 0xFF
        keys = np.full(n, 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(keys, dtype=np.uint64), vals


def sort_cases():
    """[(kind, n, nbits)]: random keys over the two full grids, the other key sets at sizes with and without a ragged
    last tile and at bit counts with 1, 2, 3 and 8 passes, the crop's fill at its 13 bits"""
    cases = [("random", n, b) for n in SORT_NBITS_AT for b in SORT_NBITS]
    cases += [("random", n, b) for b in SORT_SIZES_AT for n in SORT_SIZES if ("random", n, b) not in cases]
    for kind in SORT_KEY_SETS[1:]:
        cases += [(kind, n, b) for n in (513, 5 * TILE + 77) for b in (5, 13, 17, 64)]
    cases += [("crop_fill", n, 13) for n in (513, 5 * TILE + 77)]
    return cases


# ------------------------------------------------------------------ grouping inputs
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
GROUP_PAIRS = ([(0, 0), (0, 5000), (1, 1), (3, 0)]
               + [(K, n) for K in (254, 255) for n in (2047, 2048, 2049, 6145)]      # 255: the last one-pass K
               + [(256, 2049), (256, 70001),                    # 9 bits, 2 passes, buffer 0
                  (65535, 70001),                               # 16 bits, 2 passes
                  (65536, 70001),                               # 17 bits, 3 passes, buffer 1
                  (70001, 70001)])                              # every row its own cluster, shuffled
GROUP_PATTERNS = ("all_noise", "one_label", "alternating", "runs", "out_of_range", "empty_clusters")
GROUP_PATTERN_K = (37, 300)
GROUP_PATTERN_N = 3 * TILE + 1
BIG_K, BIG_N = 255, 10485761                     # one-pass grouping whose count table is past SCAN1_LIMIT


def group_xyz(n, seed=0):
    return np.random.default_rng([77, n, seed]).normal(0, 10, (n, 3)).astype(np.float32)


def group_labels(K, n):
    """int32 [n] for one (K, n) pair: random labels in [-1, K) with an empty cluster and a run of one label; K == n
    gives every row its own cluster, shuffled"""
    rng = np.random.default_rng([78, K, n])
    if K == n and n > 1:
        return rng.permutation(n).astype(np.int32)
    labels = rng.integers(-1, max(K, 1), n).astype(np.int32) if K else np.full(n, -1, dtype=np.int32)
    if K > 8:
        labels[labels == 5] = -1
    labels[n // 3: n // 3 + 800] = min(3, K - 1)
    return labels


def group_pattern(kind, K, n):
    rng = np.random.default_rng([79, GROUP_PATTERNS.index(kind), K, n])
    i = np.arange(n)
    if kind == "all_noise":
        return np.full(n, -1, dtype=np.int32)
    if kind == "one_label":
        return np.full(n, K - 2, dtype=np.int32)
    if kind == "alternating":                    # two bins lane by lane: no lane shares the first lane's bin run
        return np.where(i % 2 == 0, 7, K - 1).astype(np.int32)
    if kind == "runs":                           # sorted runs whose ends fall next to and across the tile edges
        cuts = np.sort(np.concatenate([rng.integers(0, n, K - 8), [TILE - 1, TILE, TILE + 1, 2 * TILE, 3 * TILE - 1]]))
        return np.searchsorted(cuts, i, side="right").astype(np.int32) - 1       # -1 .. K-4, ascending
    if kind == "out_of_range":
        labels = rng.integers(-1, K, n).astype(np.int64)
        at = rng.permutation(n)[: n // 5]
        labels[at] = np.array([K, K + 1, I32_MAX, -2, I32_MIN])[rng.integers(0, 5, len(at))]
        return labels.astype(np.int32)
    if kind == "empty_clusters":                 # empty: the first two, two neighbours in the middle, the last two
        labels = rng.integers(-1, K, n).astype(np.int32)
        for k in (0, 1, K // 2, K // 2 + 1, K - 2, K - 1):
            labels[labels == k] = 2
        return labels
    raise ValueError(kind)
