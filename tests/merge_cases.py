"""The cluster merge between stages C and D0 as a statement in plain numpy (no library import), and the seeded
builders of its tests.  The rule (include/pch_hip.h, after the reference's test/tttt.py:93-175):
  1 centre of cluster k: np.mean(P[labels == k], axis=0), NaN for a cluster without rows
  2 clusters i, j are linked iff ((dx*dx + dy*dy) + dz*dz) <= r*r in float64 on the float32 centres
  3 new id of a cluster = rank of its component, components ordered by their smallest old id
  4 labels[i] = map[labels[i]] for labels in [0, K), everything else -1
"""
import numpy as np

KS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1000]          # tile edges of the all-pairs sweep, the regrouping's 256 switch
CENTER_SIZES = [1, 2, 63, 64, 65, 127, 128, 129, 4097, 50_000]
FRAMES = {"zero": (0.0, 0.0, 0.0), "offset_5km": (5000.0, 5000.0, 80.0), "mixed_sign": (-60.0, 35.0, -3.0)}


# ---------------------------------------------------------------------------------------------------- the statement
def centers(P, labels, K):
    """(float32 [K,3], int64 [K]): live np.mean over the boolean mask of every cluster"""
    P = np.asarray(P, dtype=np.float32).reshape(-1, 3)
    out = np.full((K, 3), np.nan, dtype=np.float32)
    sizes = np.zeros((K,), dtype=np.int64)
    for k in range(K):
        rows = P[labels == k]
        sizes[k] = len(rows)
        if len(rows):
            with np.errstate(invalid="ignore", over="ignore"):
                out[k] = np.mean(rows, axis=0)
    return out, sizes


def links(C, r):
    """bool [K,K]: the reach predicate in float64, x, y, z order (NaN compares false)"""
    C = np.asarray(C, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d = C[:, None, :] - C[None, :, :]
        dist = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        return dist <= float(r) * float(r)


def merge_map(C, r):
    """(map int32 [K], nmerged): components of the link graph, numbered by their smallest member"""
    K = len(C)
    hit = links(C, r)
    comp = np.full((K,), -1, dtype=np.int64)               # smallest member of the component
    for k in range(K):
        if comp[k] >= 0:
            continue
        comp[k] = k
        todo = [k]
        while todo:
            i = todo.pop()
            for j in np.flatnonzero(hit[i] & (comp < 0)):
                comp[j] = k
                todo.append(int(j))
    roots = np.flatnonzero(comp == np.arange(K))
    rank = np.zeros((K,), dtype=np.int64)
    rank[roots] = np.arange(len(roots))
    return rank[comp].astype(np.int32), len(roots)


def relabel(labels, cmap):
    labels = np.asarray(labels, dtype=np.int32)
    K = len(cmap)
    ok = (labels >= 0) & (labels < K)
    out = np.full(labels.shape, -1, dtype=np.int32)
    out[ok] = np.asarray(cmap, dtype=np.int32)[labels[ok]]
    return out


def expected(P, labels, K, r=6.0):
    C, sizes = centers(P, labels, K)
    cmap, nmerged = merge_map(C, r)
    return dict(centers=C, sizes=sizes, map=cmap, nmerged=nmerged, labels=relabel(labels, cmap))


def canonical_bits(a):
    """uint32 view of a float32 array with every NaN set to one pattern: which NaN a 0 / 0 or an inf - inf gives (sign,
    payload) is the processor's choice, x86 and gfx950 differ, and the rule only says NaN"""
    a = np.ascontiguousarray(a, dtype=np.float32).copy()
    a[np.isnan(a)] = np.float32(np.nan)
    return a.view(np.uint32)


def map_is_ordered(cmap):
    """map[0] == 0 and map[k] <= max(map[:k]) + 1"""
    top = -1
    for v in cmap:
        if v > top + 1:
            return False
        top = max(top, int(v))
    return len(cmap) == 0 or cmap[0] == 0


# ------------------------------------------------------------------------------------------------------ the builders
def centers_cloud(frame):
    """(P float32 [n,3], labels int32 [n], K): clusters of CENTER_SIZES rows (ids 0..9), id 10 unused (empty), id 11
    with one NaN row, id 12 with one +inf row, noise rows (-1), all interleaved in file order; about 120 k rows"""
    rng = np.random.default_rng(7)
    sizes = CENTER_SIZES + [0, 300, 300]
    K = len(sizes)
    lab = np.concatenate([np.full((s,), k, dtype=np.int32) for k, s in enumerate(sizes)]
                         + [np.full((64_724,), -1, dtype=np.int32)])
    lab = lab[rng.permutation(len(lab))]
    mid = np.column_stack([rng.uniform(0, 2000, K + 1), rng.uniform(0, 100, K + 1), rng.uniform(5, 40, K + 1)])
    P = mid[lab] + rng.normal(0, 1, (len(lab), 3)) * np.array([2.5, 2.5, 9.0])
    P = (P + np.asarray(FRAMES[frame])).astype(np.float32)
    P[np.flatnonzero(lab == 11)[150], 1] = np.nan
    P[np.flatnonzero(lab == 12)[7], 2] = np.inf
    return P, lab, K


def uniform_centers(K, seed=0):
    """K centres uniform in a box sized for about 0.7 neighbours within 6 m each"""
    rng = np.random.default_rng(100 + seed)
    side = max((max(K, 1) * 905.0 / 0.7) ** (1.0 / 3.0), 1.0)
    return rng.uniform(0, side, (K, 3)).astype(np.float32)


def lattice_centers(K, seed=0):
    """even-integer lattice: pairs at distance exactly 6.0 of the (6,0,0) and (2,4,4) kind, their float32 nextafter
    neighbours just outside, then random lattice points (many more exact pairs)"""
    f = np.float32
    up = lambda v: np.nextafter(f(v), f(np.inf))
    head = [(0, 0, 0), (6, 0, 0), (100, 0, 0), (102, 4, 4), (200, 0, 0), (up(206), 0, 0), (300, 0, 0), (302, 4, up(4)),
            (400, 0, 0), (400, 6, 0), (500, 0, 0), (504, 4, 2), (600, 0, 0), (600, 0, up(6))]
    rng = np.random.default_rng(200 + seed)
    m = max(2, int(round(max(K, 1) ** (1.0 / 3.0) * 1.6)))
    tail = 2.0 * rng.integers(0, m, (max(K - len(head), 0), 3)) + np.array([0.0, 1000.0, 0.0])
    return np.vstack([np.array(head, dtype=np.float64).reshape(-1, 3), tail])[:K].astype(np.float32)


def chain_centers(chains=1):
    """300 centres 5.9 m apart per chain (ends 1.76 km apart: one component, linked only transitively); two chains lie
    6.1 m apart and take the even and the odd ids"""
    x = 5.9 * np.arange(300)
    if chains == 1:
        return np.column_stack([x, np.zeros(300), np.zeros(300)]).astype(np.float32)
    C = np.zeros((600, 3))
    C[0::2, 0], C[1::2, 0], C[1::2, 1] = x, x, 6.1
    return C.astype(np.float32)


def nan_dup_centers(K, seed=0):
    """uniform centres, every 7th one NaN (one coordinate or all three), every 5th a bit-equal copy of another"""
    C = uniform_centers(K, seed + 50)
    rng = np.random.default_rng(300 + seed)
    for k in range(K):
        if k % 7 == 3:
            C[k, rng.integers(0, 3)] = np.nan
            if k % 2:
                C[k] = np.nan
        elif k % 5 == 4:
            C[k] = C[rng.integers(0, K)]
    return C


def labels_for(K, n=3001, seed=0):
    """labels in [-3, K + 2]: noise, values outside [0, K) that must become -1, every id"""
    return np.random.default_rng(400 + seed).integers(-3, K + 3, n).astype(np.int32)


def clustered_cloud(K, seed=0):
    """(P, labels): K small clusters (1..20 rows within half a metre of uniform_centers) and noise, shuffled"""
    rng = np.random.default_rng(500 + seed)
    C = uniform_centers(K, seed + 9).astype(np.float64)
    sizes = rng.integers(1, 21, K)
    lab = np.concatenate([np.repeat(np.arange(K, dtype=np.int32), sizes), np.full((K // 2 + 5,), -1, dtype=np.int32)])
    lab = lab[rng.permutation(len(lab))]
    mid = np.vstack([C, [[0.0, 0.0, 0.0]]])
    P = (mid[lab] + rng.uniform(-0.5, 0.5, (len(lab), 3))).astype(np.float32)
    return P, lab


# ------------------------------------------------------------------------------------------ the end-to-end case
E2E = dict(chunk_size=2000, eps=8.0, min_points=20)
E2E_TOWERS = [1200, 1600, 1000, 1400]                     # kept rows 0..1199 | 1200..2799 | 2800..3799 | 3800..5199


def e2e_cloud():
    """(raw float32 [n,3], tower int32 [n]): 6000 ground rows (tower -1) and four towers 200 m apart whose rows all
    survive the height filter; in file order the towers follow each other, each shuffled inside itself, with the
    ground rows strewn between them - so with chunks of 2000 kept rows towers 1 and 3 straddle a chunk boundary
    (800 + 800 and 200 + 1200 rows) and towers 0 and 2 do not"""
    rng = np.random.default_rng(11)
    rows, who = [], []
    for t, m in enumerate(E2E_TOWERS):
        rows.append(np.column_stack([rng.normal(200.0 * t, 2.5, m), rng.normal(50.0, 2.5, m),
                                     np.clip(rng.normal(22.0, 9.0, m), 6.0, 45.0)]))
        who.append(np.full((m,), t, dtype=np.int32))
    towers, who = np.vstack(rows), np.concatenate(who)
    ng = 6000
    ground = np.column_stack([rng.uniform(-50, 650, ng), rng.uniform(0, 100, ng), rng.normal(0, 0.05, ng)])
    slot = np.sort(rng.integers(0, len(towers) + 1, ng))   # ground row g goes in front of tower row slot[g]
    order = np.argsort(np.concatenate([np.arange(len(towers)) + 0.5, slot.astype(np.float64)]), kind="stable")
    raw = np.vstack([towers, ground])[order] + np.array([437000.0, 3139000.0, 80.0])
    return raw.astype(np.float32), np.concatenate([who, np.full((ng,), -1, dtype=np.int32)])[order]
