"""The statement of pch_crop_boxes_f64 and the clouds and boxes its tests use (TEST INFRASTRUCTURE, pure numpy;
imported by the CPU and the GPU tests, not a conftest).

``inside`` says which rows a box takes: both predicates of include/pch_hip.h restated with elementwise numpy only -
never ``@``, whose BLAS kernels may fuse a product into a sum, and the comparison with the library is bit for bit.
``expected`` says what ``ops.crop_boxes`` returns.  Boxes are the tuples ``ops.crop_boxes`` takes:
("aabb", lo, hi) and ("obb", center, rotation, extent) with the box axes in the COLUMNS of rotation and extent the
full side lengths (half = extent * 0.5, exact).
"""
import numpy as np

OFFSET = np.array([437000.0, 3139000.0, 80.0])
SPAN = np.array([400.0, 100.0, 60.0])


# ------------------------------------------------------------------ the statement
def inside_aabb(P, lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return ((P[:, 0] >= lo[0]) & (P[:, 0] <= hi[0]) & (P[:, 1] >= lo[1]) & (P[:, 1] <= hi[1])
                & (P[:, 2] >= lo[2]) & (P[:, 2] <= hi[2]))


def inside_obb(P, center, R, half):
    c, R, h = (np.asarray(v, dtype=np.float64) for v in (center, R, half))
    R = R.reshape(3, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        d0, d1, d2 = P[:, 0] - c[0], P[:, 1] - c[1], P[:, 2] - c[2]
        u0 = (d0 * R[0, 0] + d1 * R[1, 0]) + d2 * R[2, 0]
        u1 = (d0 * R[0, 1] + d1 * R[1, 1]) + d2 * R[2, 1]
        u2 = (d0 * R[0, 2] + d1 * R[1, 2]) + d2 * R[2, 2]
        return ((u0 >= -h[0]) & (u0 <= h[0]) & (u1 >= -h[1]) & (u1 <= h[1]) & (u2 >= -h[2]) & (u2 <= h[2]))


def inside(P, box):
    if box[0] == "aabb":
        return inside_aabb(P, box[1], box[2])
    assert box[0] == "obb"
    return inside_obb(P, box[1], box[2], np.asarray(box[3], dtype=np.float64) * 0.5)


def expected(P, boxes):
    """(points [M,3], index int64 [M], offsets int64 [T+1]): per box, in box order, points[mask] and its rows"""
    rows = [np.flatnonzero(inside(P, b)) for b in boxes]
    index = np.concatenate(rows).astype(np.int64) if rows else np.zeros((0,), dtype=np.int64)
    offsets = np.zeros(len(boxes) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(r) for r in rows])
    return P[index], index, offsets


# ------------------------------------------------------------------ clouds
def cloud(n, seed=None):
    """float64 [n,3]: uniform in 400 x 100 x 60 m plus OFFSET, a quarter of the rows rounded to whole metres (many sit
    exactly ON a bound of the boxes below), one row holding NaN and one holding +inf (n > 10)"""
    rng = np.random.default_rng(n + 1 if seed is None else seed)
    P = rng.random((n, 3)) * SPAN + OFFSET
    P[: n // 4] = np.round(P[: n // 4], 0)
    if n > 10:
        P[5, 1] = np.nan
        P[n - 3, 0] = np.inf
    return P


def x_sorted(P):
    """P in ascending x (NaN / inf rows last): the spatially coherent order of a file"""
    return P[np.argsort(P[:, 0], kind="stable")]


# ------------------------------------------------------------------ rotations
def rot_z(deg):
    a = np.deg2rad(deg)
    return np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])


def random_rotation(rng):
    """QR of a Gaussian matrix, determinant fixed to +1"""
    Q, Rr = np.linalg.qr(rng.normal(size=(3, 3)))
    Q = Q * np.sign(np.diag(Rr))[None, :]
    if np.linalg.det(Q) < 0:
        Q[:, 2] = -Q[:, 2]
    return Q


def named_rotations():
    """0 deg, 90 deg about z (exact entries), an axis permutation, 30 deg about z, a general rotation"""
    r90 = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    perm = np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    return [np.eye(3), r90, perm, rot_z(30.0), random_rotation(np.random.default_rng(5))]


# ------------------------------------------------------------------ boxes
def kuangxuan_box(c, w, h):
    """the reference's own arithmetic (test/kuangxuan.py:60-68): c - w/1, c + w/0.6, ..."""
    lo = np.array([c[0] - w / 1, c[1] - w / 2, c[2] - h / 1])
    hi = np.array([c[0] + w / 0.6, c[1] + w / 1, c[2] + h * 2])
    return ("aabb", lo, hi)


def special_boxes():
    """The box mix of every case with 33 boxes or more, 23 boxes: two overlapping boxes, the same box twice, a box
    with lo > hi, a box with a NaN bound, a box covering everything (infinite bounds: it takes the +inf row, as the
    numpy mask does), a finite box covering every finite row, a box far outside, three kuangxuan boxes (one with
    bounds rounded to whole metres, so that rounded rows lie ON it); five oriented boxes (the named rotations) whose
    centre and half extents are whole metres - for the three exact rotations the rounded rows lie exactly on their
    faces; an oriented box with a NaN in axes, one with a NaN centre, one with infinite half extents, one with
    negative half extents, one whose axes are far from orthonormal, and the same oriented box twice."""
    c = OFFSET + [200.0, 50.0, 20.0]
    k1 = kuangxuan_box(c, 40.0, 15.0)
    k2 = kuangxuan_box(OFFSET + [90.0, 30.0, 10.0], 20.1, 17.4)
    k3 = ("aabb", np.round(k1[1]), np.round(k1[2]))
    over_a = ("aabb", OFFSET + [100.0, 20.0, 5.0], OFFSET + [160.0, 70.0, 40.0])
    over_b = ("aabb", OFFSET + [140.0, 40.0, 0.0], OFFSET + [220.0, 90.0, 30.0])
    out = [over_a, over_b, k1, k1,
           ("aabb", OFFSET + [300.0, 60.0, 30.0], OFFSET + [250.0, 90.0, 50.0]),               # lo > hi
           ("aabb", OFFSET + [100.0, np.nan, 0.0], OFFSET + [300.0, 90.0, 50.0]),              # NaN bound
           ("aabb", [-np.inf] * 3, [np.inf] * 3),                                              # everything
           ("aabb", OFFSET - 1.0, OFFSET + SPAN + 1.0),                                        # every finite row
           ("aabb", [1e9] * 3, [2e9] * 3),                                                     # far outside
           k2, k3]
    for k, R in enumerate(named_rotations()):
        out.append(("obb", OFFSET + [60.0 + 70.0 * k, 50.0, 30.0], R, np.array([40.0, 24.0, 30.0])))
    bad = named_rotations()[3].copy()
    bad[1, 2] = np.nan
    ob = ("obb", OFFSET + [250.0, 40.0, 25.0], rot_z(30.0), np.array([50.0, 30.0, 40.0]))
    out += [("obb", OFFSET + [200.0, 50.0, 30.0], bad, np.array([60.0, 60.0, 60.0])),          # NaN in axes
            ("obb", OFFSET + [np.nan, 50.0, 30.0], np.eye(3), np.array([60.0, 60.0, 60.0])),   # NaN centre
            ("obb", OFFSET + [200.0, 50.0, 30.0], rot_z(30.0), np.array([np.inf] * 3)),        # everything finite
            ("obb", OFFSET + [200.0, 50.0, 30.0], rot_z(30.0), np.array([-10.0, 20.0, 20.0])),  # empty
            ("obb", OFFSET + [200.0, 50.0, 30.0], rot_z(30.0) * [[0.25, 1.0, 3.0]], np.array([30.0, 30.0, 30.0])),
            ob, ob]
    return out


def random_box(rng):
    """a small box somewhere in (or a little outside) the cloud's span: three in four axis-aligned, some with whole
    metre bounds"""
    c = OFFSET + rng.uniform(-0.1, 1.1, 3) * SPAN
    e = rng.uniform(2.0, 40.0, 3)
    kind = rng.integers(0, 4)
    if kind == 0:
        return ("obb", c, random_rotation(rng), e)
    if kind == 1:
        return ("aabb", np.round(c - e / 2), np.round(c + e / 2))
    return ("aabb", c - e / 2, c + e / 2)


def special_positions(T, seed=0):
    """where box_mix(T, seed) puts special_boxes(), in their order (ascending)"""
    rng = np.random.default_rng(2000 + T + seed)
    return np.sort(rng.choice(T, len(special_boxes()), replace=False))


def box_mix(T, seed=0):
    """T boxes.  1: a kuangxuan box; 2: two overlapping boxes, one of either kind; 33 and more: special_boxes() at
    seeded positions among seeded random boxes"""
    c = OFFSET + [200.0, 50.0, 20.0]
    if T == 0:
        return []
    if T == 1:
        return [kuangxuan_box(c, 40.0, 15.0)]
    if T == 2:
        return [kuangxuan_box(c, 40.0, 15.0), ("obb", c + [30.0, 0.0, 10.0], rot_z(30.0), np.array([80.0, 40.0, 50.0]))]
    rng = np.random.default_rng(1000 + T + seed)
    sp = special_boxes()
    assert T >= len(sp)
    boxes = [random_box(rng) for _ in range(T)]
    for at, b in zip(special_positions(T, seed), sp):
        boxes[at] = b
    return boxes


def full_x_boxes(T, seed=3):
    """T boxes that each span the whole x range of the cloud (every tile of an x-sorted cloud meets every box): slabs
    in y and z, every fourth one oriented about x's own axis"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(T):
        y0, z0 = rng.uniform(0.0, 90.0), rng.uniform(0.0, 50.0)
        if t % 4 == 3:
            a = np.deg2rad(rng.uniform(0.0, 90.0))
            R = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(a), -np.sin(a)], [0.0, np.sin(a), np.cos(a)]])
            out.append(("obb", OFFSET + [200.0, y0 + 5.0, z0 + 5.0], R, np.array([500.0, 8.0, 6.0])))
        else:
            out.append(("aabb", OFFSET + [-10.0, y0, z0], OFFSET + [410.0, y0 + rng.uniform(1.0, 6.0), z0 + 4.0]))
    return out


def far_boxes(T=33, seed=4):
    """T finite boxes of both kinds, all outside the cloud: no tile meets any"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(T):
        c = OFFSET + [600.0 + 50.0 * t, rng.uniform(-500.0, 500.0), rng.uniform(100.0, 300.0)]
        e = rng.uniform(5.0, 40.0, 3)
        out.append(("obb", c, random_rotation(rng), e) if t % 2 else ("aabb", c - e / 2, c + e / 2))
    return out
