"""The all-pairs statement of pch_dbscan_kdist_f32, of pipeline.kdistance_knee, and the cloud of the k-distance tests
that no on-chip buffer holds (TEST INFRASTRUCTURE, pure numpy; imported by the CPU and the GPU tests, not a conftest).

``kdist_reference`` says what ``ops.DbscanFit.kdist`` returns: per query the k-th smallest ``dbscan_cases.pair_d2``
(float64, three squares accumulated in order) among the fit's rows of the query's chunk that lie within ``eps*eps``,
``+inf`` if there are fewer than k, and how many there are.  Nothing here knows about cells, keys, pieces or digits.
"""
import numpy as np

import dbscan_cases as dc


# ------------------------------------------------------------------ the statement
def kdist_reference(X, Q, eps, k, chunk_size=0, query_chunk=None, sub=None, block=512):
    """(d2 float64, count int32 [len(Q)]).  ``k`` is one rank (d2 is [len(Q)]) or a sequence of ranks (d2 is [len(k),
    len(Q)]: one pass over the matrix serves them all).  X: the fitted rows, all of them count, core or not.
    q = float32(Q) - float32(sub), a float32 subtraction.  chunk_size > 0: one fit per chunk_size rows, query_chunk[i]
    names the chunk query i is held against; an index outside [0, nchunks), a chunk holding NaN/inf and a query holding
    NaN/inf give count 0 and +inf."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32)).reshape(-1, 3)
    q = np.ascontiguousarray(np.asarray(Q, dtype=np.float32)).reshape(-1, 3)
    if sub is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            q = q - np.asarray(sub, dtype=np.float32)[None, :]
        assert q.dtype == np.float32
    one = np.ndim(k) == 0
    ks = np.atleast_1d(np.asarray(k, dtype=np.int64))
    assert (ks >= 1).all()
    n, nq = len(X), len(q)
    cs = int(chunk_size) if 0 < int(chunk_size) < n else max(n, 1)
    nchunks = max(-(-n // cs), 1)
    if query_chunk is None:
        assert nchunks == 1, "a chunked fit needs query_chunk"
        qc = np.zeros(nq, dtype=np.int64)
    else:
        qc = np.asarray(query_chunk).astype(np.int64)
    d2 = np.full((len(ks), nq), np.inf, dtype=np.float64)
    count = np.zeros(nq, dtype=np.int32)
    r2 = float(eps) * float(eps)
    finite_q = np.isfinite(q).all(1)
    for c in range(nchunks):
        lo, hi = c * cs, min((c + 1) * cs, n)
        if hi <= lo or not np.isfinite(X[lo:hi]).all():            # sklearn refuses the chunk: no fit
            continue
        q_rows = np.flatnonzero((qc == c) & finite_q)
        have = ks <= hi - lo                                       # a rank beyond the chunk's rows: +inf
        kth = np.unique(ks[have] - 1)
        for s in range(0, len(q_rows), block):
            part = q_rows[s:s + block]
            D = dc.pair_d2(X[lo:hi], q[part])
            inside = D <= r2
            count[part] = inside.sum(1)
            if not len(kth):
                continue
            D[~inside] = np.inf
            P = np.partition(D, kth, axis=1)                       # P[:, j] is the (j+1)-th smallest for j in kth
            for a in np.flatnonzero(have):
                d2[a, part] = P[:, ks[a] - 1]
    assert np.array_equal(np.isfinite(d2), count[None, :] >= ks[:, None])
    return (d2[0] if one else d2), count


def knee_reference(y):
    """pipeline.kdistance_knee by its definition, one element at a time"""
    y = [float(v) for v in y]
    m = len(y)
    if m < 3:
        return None
    if y[-1] == y[0]:
        return y[0]
    best, arg = None, 0
    for i in range(m):
        gap = i / (m - 1) - (y[i] - y[0]) / (y[-1] - y[0])
        if best is None or gap > best:
            best, arg = gap, i
    return y[arg]


# ------------------------------------------------------------------ a neighbourhood beyond any on-chip buffer
BIG_EPS = 1.0
BIG_KS = (1, 2, 64, 65, 1500, 4096, 6015, 6016)
_BIG = {}


def big_cloud():
    """(X float32 [9000,3], query rows int64 [512]).  6 000 rows of normal(0, 0.12) - a clump far inside eps = 1 of
    itself, so a row of it has some 6 000 rows in reach - of which rows 0..1499 are copies of rows 1500..2999 (equal
    d2 in every neighbourhood: ties at every rank), and 3 000 rows of uniform(-6, 6); shuffled.  The queries are 512
    seeded rows of the cloud."""
    if not _BIG:
        rng = np.random.default_rng(11)
        A = rng.normal(0.0, 0.12, (6000, 3))
        A[:1500] = A[1500:3000]
        B = rng.uniform(-6.0, 6.0, (3000, 3))
        X = np.vstack([A, B]).astype(np.float32)
        X = X[rng.permutation(len(X))]
        rows = np.sort(rng.choice(len(X), 512, replace=False)).astype(np.int64)
        X.setflags(write=False)
        rows.setflags(write=False)
        _BIG["case"] = (X, rows)
    return _BIG["case"]
