"""The all-pairs statement of pch_dbscan_shape_f32, the eigenvalue features by LAPACK, and the corridor scene of the
wire-removal tests (TEST INFRASTRUCTURE, pure numpy; imported by the CPU and the GPU tests, not a conftest).

``shape_reference`` says what ``ops.DbscanFit.shape`` returns: per query the number of the fit's rows of the query's
chunk with ``d2 <= radius*radius`` (float64, three squares accumulated in x, y, z order - ``dbscan_cases.pair_d2``'s
number) and the nine sums of their differences ``row - query``.  Nothing here knows about cells, keys, pieces or waves.
"""
import numpy as np

U = 2.0 ** -53                                   # unit roundoff of float64


# ------------------------------------------------------------------ the statement
def shape_reference(X, Q, radius, chunk_size=0, query_chunk=None, sub=None, block=256):
    """(count int32 [nq], moments float64 [nq, 9]).  X: the fitted rows, all of them count, core or not.
    q = float32(Q) - float32(sub), a float32 subtraction.  d = float64(row) - float64(q) per component (exact);
    d2 = (dx*dx + dy*dy) + dz*dz; a row is in when d2 <= radius*radius.  moments = (Σdx, Σdy, Σdz, Σdx², Σdy², Σdz²,
    Σdx·dy, Σdx·dz, Σdy·dz) over the rows that are in, float64 sums (numpy's order).  chunk_size > 0: one fit per
    chunk_size rows, query_chunk[i] names the chunk query i is held against; an index outside [0, nchunks), a chunk
    holding NaN/inf and a query holding NaN/inf give count 0 and nine zeros."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float32)).reshape(-1, 3)
    q = np.ascontiguousarray(np.asarray(Q, dtype=np.float32)).reshape(-1, 3)
    if sub is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            q = q - np.asarray(sub, dtype=np.float32)[None, :]
        assert q.dtype == np.float32
    n, nq = len(X), len(q)
    cs = int(chunk_size) if 0 < int(chunk_size) < n else max(n, 1)
    nchunks = max(-(-n // cs), 1)
    if query_chunk is None:
        assert nchunks == 1, "a chunked fit needs query_chunk"
        qc = np.zeros(nq, dtype=np.int64)
    else:
        qc = np.asarray(query_chunk).astype(np.int64)
    count = np.zeros(nq, dtype=np.int32)
    moments = np.zeros((nq, 9), dtype=np.float64)
    r2 = float(radius) * float(radius)
    finite_q = np.isfinite(q).all(1)
    for c in range(nchunks):
        lo, hi = c * cs, min((c + 1) * cs, n)
        if hi <= lo or not np.isfinite(X[lo:hi]).all():            # sklearn refuses the chunk: no fit
            continue
        q_rows = np.flatnonzero((qc == c) & finite_q)
        X64 = X[lo:hi].astype(np.float64)
        for s in range(0, len(q_rows), block):
            part = q_rows[s:s + block]
            d = X64[None, :, :] - q[part].astype(np.float64)[:, None, :]
            dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
            d2 = dx * dx
            d2 += dy * dy
            d2 += dz * dz
            inside = d2 <= r2
            count[part] = inside.sum(1)
            for a, t in enumerate((dx, dy, dz, dx * dx, dy * dy, dz * dz, dx * dy, dx * dz, dy * dz)):
                moments[part, a] = np.where(inside, t, 0.0).sum(1)
    return count, moments


def moment_bounds(count, radius):
    """[nq, 9] how far a moment may lie from the reference's: sums of the same n terms in another order, or with fused
    products, differ by at most (n+1)·u·Σ|t| each, and Σ|t| <= n·r for a difference, n·r² for a product of two; two
    such sums are compared, hence the factor 2"""
    n = np.asarray(count, dtype=np.float64)
    r = float(radius)
    first = 2.0 * (n + 1.0) * U * n * r
    second = 2.0 * (n + 1.0) * U * n * r * r
    return np.stack([first] * 3 + [second] * 6, axis=1)


def covariance(count, moments):
    """([nq,3,3] C = M2/n - mu mu^T with n = max(count, 1), [nq] trace) in float64"""
    n = np.maximum(np.asarray(count, dtype=np.float64), 1.0)
    M = np.asarray(moments, dtype=np.float64).reshape(-1, 9)
    mu = M[:, 0:3] / n[:, None]
    C = np.empty((len(M), 3, 3), dtype=np.float64)
    for (i, j), a in {(0, 0): 3, (1, 1): 4, (2, 2): 5, (0, 1): 6, (0, 2): 7, (1, 2): 8}.items():
        C[:, i, j] = C[:, j, i] = M[:, a] / n - mu[:, i] * mu[:, j]
    return C, np.trace(C, axis1=1, axis2=2)


def features_reference(count, moments):
    """dict of float64 [nq]: l1 >= l2 >= l3 (np.linalg.eigh of ``covariance``), verticality |e1.z|, linearity,
    planarity, scattering (0 where l1 <= 0), trace"""
    C, trace = covariance(count, moments)
    w, V = np.linalg.eigh(C)                                     # ascending
    l1, l2, l3 = w[:, 2], w[:, 1], w[:, 0]
    ok = l1 > 0
    den = np.where(ok, l1, 1.0)
    return dict(l1=l1, l2=l2, l3=l3, verticality=np.abs(V[:, 2, 2]), trace=trace,
                linearity=np.where(ok, (l1 - l2) / den, 0.0), planarity=np.where(ok, (l2 - l3) / den, 0.0),
                scattering=np.where(ok, l3 / den, 0.0))


def drop_mask_reference(X, radius=2.0, linearity=0.9, verticality=0.5, min_rows=10):
    """(mask of the rows pipeline.drop_linear_rows drops, features, count) by the reference"""
    count, moments = shape_reference(X, X, radius)
    f = features_reference(count, moments)
    return (f["linearity"] >= linearity) & (f["verticality"] <= verticality) & (count >= min_rows), f, count


# ------------------------------------------------------------------ the scene: two towers joined by three conductors
SCENE_ROWS, SCENE_WIRE_ROWS = 6803, 1803
SCENE_RULE = dict(radius=2.0, linearity=0.9, verticality=0.5, min_rows=10)
_SCENE = {}


def scene():
    """(X float32 [6803,3], wire bool [6803], x0 float64 [6803]: the x a row was generated at).  Two towers at x = 0
    and 60: 2000 rows uniform in a column 0..30 m high whose half-width tapers from 4 m to 1 m, and 500 rows of a
    cross-arm uniform in [+-1] x [+-8] x [25, 27].  Three conductors at y = -7, 0, +7: one row every 0.1 m of x from 0
    to 60, z = 26 - 3(1 - (2x/60 - 1)^2), N(0, 0.02) jitter per coordinate.  Cast to float32, then permuted."""
    if not _SCENE:
        rng = np.random.default_rng(0)
        parts, wire = [], []
        for cx in (0.0, 60.0):
            z = rng.uniform(0.0, 30.0, 2000)
            hw = 4.0 - 3.0 * z / 30.0
            col = np.stack([cx + rng.uniform(-1.0, 1.0, 2000) * hw, rng.uniform(-1.0, 1.0, 2000) * hw, z], axis=1)
            arm = np.stack([cx + rng.uniform(-1.0, 1.0, 500), rng.uniform(-8.0, 8.0, 500),
                            rng.uniform(25.0, 27.0, 500)], axis=1)
            parts += [col, arm]
            wire += [np.zeros(2500, dtype=bool)]
        x = np.arange(601) * 0.1
        for y in (-7.0, 0.0, 7.0):
            line = np.stack([x, np.full_like(x, y), 26.0 - 3.0 * (1.0 - (2.0 * x / 60.0 - 1.0) ** 2)], axis=1)
            parts.append(line + rng.normal(0.0, 0.02, line.shape))
            wire.append(np.ones(len(x), dtype=bool))
        P = np.vstack(parts)
        wire = np.concatenate(wire)
        x0 = np.concatenate([P[:5000, 0], x, x, x])
        perm = rng.permutation(len(P))
        X = P.astype(np.float32)[perm]
        wire, x0 = wire[perm], x0[perm]
        for a in (X, wire, x0):
            a.setflags(write=False)
        _SCENE["case"] = (X, wire, x0)
    return _SCENE["case"]


def scene_with_ground(seed=1, rows=20000):
    """the scene lifted so that a sheet of ground rows below it takes the percentile: float32 [6803 + rows, 3], the
    scene's rows first.  The sheet lies at z in [0, 0.2] under the whole span, the scene's feet start 3.5 m above it, so
    the default rule (25th percentile + 3 m) keeps exactly the scene's rows."""
    X, _, _ = scene()
    rng = np.random.default_rng(seed)
    sheet = np.stack([rng.uniform(-10.0, 70.0, rows), rng.uniform(-10.0, 10.0, rows), rng.uniform(0.0, 0.2, rows)],
                     axis=1).astype(np.float32)
    lifted = X.copy()
    lifted[:, 2] += np.float32(3.5)
    return np.vstack([lifted, sheet])
