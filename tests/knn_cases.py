"""The all-pairs statement of pch_dbscan_knn_f32, the sparse-row drop by its definition, and the corridor scene with
stray returns (TEST INFRASTRUCTURE, pure numpy; imported by the CPU and the GPU tests, not a conftest).

``knn_reference`` says what ``ops.DbscanFit.knn`` returns: per query the rows of the query's chunk with
``dbscan_cases.pair_d2 <= eps*eps`` in ``(d2, row)`` order - a stable sort of the matrix row, whose columns are the
chunk's rows in file order -, the first k of them with their d2, ``-1`` / ``+inf`` behind them, and how many there are.
Rows are global.  Nothing here knows about cells, keys, pieces or digits.
"""
import numpy as np

import dbscan_cases as dc
import shape_cases as sc

U = 2.0 ** -53                                   # unit roundoff of float64


# ------------------------------------------------------------------ the statement
def knn_reference(X, Q, eps, k, chunk_size=0, query_chunk=None, sub=None, block=256, literal=False):
    """(rows int32 [nq,k], d2 float64 [nq,k], count int32 [nq]).  X: the fitted rows, all of them count, core or not.
    q = float32(Q) - float32(sub), a float32 subtraction.  chunk_size > 0: one fit per chunk_size rows, query_chunk[i]
    names the chunk query i is held against; an index outside [0, nchunks), a chunk holding NaN/inf and a query holding
    NaN/inf give count 0 and k empty slots (-1, +inf).  ``literal``: order every matrix row by one stable argsort, the
    statement word for word; the default orders only the entries up to the k-th smallest value, which gives the same
    answer (test_knn_host.py compares the two) in a fraction of the time."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32)).reshape(-1, 3)
    q = np.ascontiguousarray(np.asarray(Q, dtype=np.float32)).reshape(-1, 3)
    if sub is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            q = q - np.asarray(sub, dtype=np.float32)[None, :]
        assert q.dtype == np.float32
    k = int(k)
    assert k >= 1
    n, nq = len(X), len(q)
    cs = int(chunk_size) if 0 < int(chunk_size) < n else max(n, 1)
    nchunks = max(-(-n // cs), 1)
    if query_chunk is None:
        assert nchunks == 1, "a chunked fit needs query_chunk"
        qc = np.zeros(nq, dtype=np.int64)
    else:
        qc = np.asarray(query_chunk).astype(np.int64)
    rows = np.full((nq, k), -1, dtype=np.int32)
    d2 = np.full((nq, k), np.inf, dtype=np.float64)
    count = np.zeros(nq, dtype=np.int32)
    r2 = float(eps) * float(eps)
    finite_q = np.isfinite(q).all(1)
    for c in range(nchunks):
        lo, hi = c * cs, min((c + 1) * cs, n)
        if hi <= lo or not np.isfinite(X[lo:hi]).all():            # sklearn refuses the chunk: no fit
            continue
        q_rows = np.flatnonzero((qc == c) & finite_q)
        kk = min(k, hi - lo)
        for s in range(0, len(q_rows), block):
            part = q_rows[s:s + block]
            D = dc.pair_d2(X[lo:hi], q[part])
            inside = D <= r2
            count[part] = inside.sum(1)
            D[~inside] = np.inf
            if literal:
                order = np.argsort(D, axis=1, kind="stable")[:, :kk]   # ties by column = by row
                near = np.take_along_axis(D, order, axis=1)
                d2[part, :kk] = near
                rows[part, :kk] = np.where(np.isfinite(near), order + lo, -1)
                continue
            # the same answer without sorting whole matrix rows: nothing beyond the kk-th smallest value can be among
            # the first kk of the stable order, so only the entries up to it are ordered, by (query, d2, column)
            kth = np.partition(D, kk - 1, axis=1)[:, kk - 1]
            i, j = np.nonzero(inside & (D <= kth[:, None]))
            v = D[i, j]
            o = np.lexsort((j, v, i))
            i, j, v = i[o], j[o], v[o]
            pos = np.arange(len(i)) - np.searchsorted(i, np.arange(len(part)))[i]
            keep = pos < kk
            d2[part[i[keep]], pos[keep]] = v[keep]
            rows[part[i[keep]], pos[keep]] = j[keep] + lo
    assert np.array_equal(np.isfinite(d2), np.arange(k)[None, :] < count[:, None])
    assert np.array_equal(rows >= 0, np.isfinite(d2))
    return rows, d2, count


def mean_distance_reference(d2, count, k):
    """ops.knn_mean_distance by its definition: the roots summed sequentially over ascending slots, divided once;
    +inf where count < k"""
    d2 = np.asarray(d2, dtype=np.float64)
    m = np.full(len(d2), np.inf, dtype=np.float64)
    full = np.asarray(count) >= k
    acc = np.zeros(int(full.sum()), dtype=np.float64)
    for j in range(k):
        acc = acc + np.sqrt(d2[full, j])
    m[full] = acc / float(k)
    return m


def mean_distance_bound(k):
    """relative distance allowed between two evaluations of sum_j sqrt(d2_j) / k: each sums k non-negative roots, every
    root within 1 ulp of the exact one, in some order (k - 1 roundings) and divides once (1 rounding), so each lies
    within (k + 4)·2^-53 relative of the exact value (second-order terms included), and two of them within twice that"""
    return 2.0 * (k + 4) * U


def sparse_reference(X, k, radius, std_ratio):
    """pipeline.drop_sparse_rows by its definition: dict(dropped, m, count, threshold, by_count, by_mean, margin).
    margin: the smallest relative distance of any finite mean from the threshold"""
    X = np.asarray(X, dtype=np.float32)
    _, d2, count = knn_reference(X, X, radius, k)
    m = mean_distance_reference(d2, count, k)
    full = count >= k
    thr = np.inf
    if full.sum() >= 2:
        thr = float(m[full].mean() + float(std_ratio) * m[full].std(ddof=1))
    by_count, by_mean = ~full, full & (m > thr)
    margin = float(np.abs(m[full] - thr).min() / thr) if np.isfinite(thr) else np.inf
    return dict(dropped=by_count | by_mean, m=m, count=count, threshold=thr, by_count=by_count, by_mean=by_mean,
                margin=margin)


def threshold_bound(n, k, radius, std_ratio):
    """how far the threshold of two evaluations of the rule may lie apart, absolute.  N = n rows with count >= k, every
    mean m_i in [0, R], the two sides' means within d = mean_distance_bound(k) relative of each other, both sides in
    two passes (sum / N; sqrt(sum((m - mu)^2) / (N - 1))), sums of non-negative terms in any order, u = 2^-53:
      mu: a sum of N non-negative terms errs by at most (N - 1)u relative, the division by u: each side's mu within
          N·u·R of the exact mean of its inputs, the inputs within d·R: |mu_a - mu_b| <= (2N·u + d)·R;
      sd: the exact sd is sqrt(N/(N-1))-Lipschitz in the largest input difference: 2d·R.  A side's own arithmetic:
          the mean it subtracts is off by e <= N·u·R, which adds N·e^2 to the sum of squares, at most sqrt(N/(N-1))·e
          <= 2N·u·R to sd; the subtraction, square, sum, division and root err by at most (N + 6)u/2 relative on sd
          <= R.  Per side 3(N + 2)u·R: |sd_a - sd_b| <= (6(N + 2)u + 2d)·R;
      thr = mu + s·sd: two more roundings per side, 4u(1 + |s|)·R.
    Together |thr_a - thr_b| <= (1 + |s|)·(6(N + 3)u + 2d)·R."""
    return (1.0 + abs(float(std_ratio))) * (6.0 * (n + 3) * U + 2.0 * mean_distance_bound(k)) * float(radius)


# ------------------------------------------------------------------ the scene with stray returns
STRAY_ROWS, N_STRAYS = 6963, 160
SPARSE_RULES = (dict(k=8, radius=2.0, std_ratio=2.0), dict(k=8, radius=2.0, std_ratio=3.0))
_STRAYS = {}


def scene_with_strays():
    """(X float32 [6963,3], kind int8 [6963]: 0 tower / 1 wire / 2 stray).  shape_cases.scene() plus 150 stray rows
    uniform in [-10, 70] x [-12, 12] x [0, 45] and 10 rows that pair up with the first ten of them (N(0, 0.1) per
    coordinate); cast to float32, then one permutation for both."""
    if not _STRAYS:
        X, wire, _ = sc.scene()
        rng = np.random.default_rng(2)
        stray = np.stack([rng.uniform(-10.0, 70.0, 150), rng.uniform(-12.0, 12.0, 150), rng.uniform(0.0, 45.0, 150)],
                         axis=1)
        pairs = stray[:10] + rng.normal(0.0, 0.1, (10, 3))
        P = np.vstack([X, stray.astype(np.float32), pairs.astype(np.float32)])
        kind = np.concatenate([wire.astype(np.int8), np.full(N_STRAYS, 2, dtype=np.int8)])
        perm = rng.permutation(len(P))
        P, kind = P[perm], kind[perm]
        assert P.dtype == np.float32 and P.shape == (STRAY_ROWS, 3)
        for a in (P, kind):
            a.setflags(write=False)
        _STRAYS["case"] = (P, kind)
    return _STRAYS["case"]


def strays_with_ground(seed=1, rows=20000):
    """the strays scene lifted above a sheet of ground rows, built the way shape_cases.scene_with_ground builds from
    the scene: float32 [6963 + rows, 3], the scene's rows first.  Every row of the scene, strays included, lies at
    least 3.5 m above the sheet, so the default rule (25th percentile + 3 m) keeps exactly the scene's rows."""
    X, _ = scene_with_strays()
    rng = np.random.default_rng(seed)
    sheet = np.stack([rng.uniform(-10.0, 70.0, rows), rng.uniform(-10.0, 10.0, rows), rng.uniform(0.0, 0.2, rows)],
                     axis=1).astype(np.float32)
    lifted = X.copy()
    lifted[:, 2] += np.float32(3.5)
    return np.vstack([lifted, sheet])


_SPARSE = {}


def sparse_case(rule_no):
    """sparse_reference of the strays scene at SPARSE_RULES[rule_no], computed once per process"""
    if rule_no not in _SPARSE:
        X, _ = scene_with_strays()
        _SPARSE[rule_no] = sparse_reference(X, **SPARSE_RULES[rule_no])
    return _SPARSE[rule_no]
