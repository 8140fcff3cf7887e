"""Wind swing clearance: the numpy statement of include/pch_hip.h's rule - tables, per row and span, per span -, a
second, vectorised statement (whole [n,S] arrays per span, the winner by argmin), a dense-angle brute force over 2001
angles with the same polyline distance, the rule's boundary rows on dyadic values, random sloped spans, and the scene:
``clearance_cases.tree_scene`` with objects that tell a swung wire from one at rest (TEST INFRASTRUCTURE, pure numpy;
imported by the CPU and the GPU tests, not a conftest).  The statement loops spans and segments over all rows; nothing
here knows about tiles, bounds or culling."""
import numpy as np

import clearance_cases as cc
import shape_cases as sc
import span_cases as sp

OUTPUTS = ("dist2", "span", "sin", "count", "violations", "min_dist2", "min_row")
TURN = 1e-6                                         # |sT*sT + cT*cT - 1| of a span that takes part


# ------------------------------------------------------------------ tables
def heads_reference(curves, angle_deg):
    """float64 [K,11] = (cx, cy, cz, ux, uy, mA, mB, zA, kap, sT, cT), one loop per span; the vertices z_0 and z_S are
    the clearance rule's (m_0 = m0, m_S = m1)"""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 10)
    K = len(curves)
    ang = np.broadcast_to(np.asarray(angle_deg, dtype=np.float64), (K,))
    heads = np.zeros((K, 11), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(K):
            a, b, c, m0, m1 = curves[k, 5:10]
            z0, z1 = a + m0 * (b + c * m0), a + m1 * (b + c * m1)
            kap = (z1 - z0) / (m1 - m0)
            rad = np.radians(ang[k])
            heads[k] = tuple(curves[k, :5]) + (m0, m1, z0, kap, np.sin(rad), np.cos(rad))
    return heads


def segments_reference(curves, S):
    """float64 [K,S,6] = (m_j, z_j, f_j, dm_j, dz_j, df_j), one loop per span and vertex; m_j and z_j are exactly
    ``clearance_cases.segments_reference``'s"""
    curves = np.asarray(curves, dtype=np.float64).reshape(-1, 10)
    K = len(curves)
    segs = np.zeros((K, S, 6), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(K):
            a, b, c, m0, m1 = curves[k, 5:10]
            step = (m1 - m0) / float(S)
            m = np.array([m0 + float(j) * step for j in range(S)] + [m1])
            z = np.array([a + mj * (b + c * mj) for mj in m])
            kap = (z[S] - z[0]) / (m[S] - m[0])
            f = np.array([(z[0] + ((m[j] - m[0]) * kap)) - z[j] for j in range(S + 1)])
            for j in range(S):
                segs[k, j] = (m[j], z[j], f[j], m[j + 1] - m[j], z[j + 1] - z[j], f[j + 1] - f[j])
    return segs


def takes_part(heads, segs):
    """bool [K]: all 11 + 6 S values finite, mB > mA, 0 <= sT <= 1, 0 < cT <= 1, |((sT*sT) + (cT*cT)) - 1| <= 1e-6"""
    heads, segs = np.asarray(heads, dtype=np.float64), np.asarray(segs, dtype=np.float64)
    out = np.zeros(len(heads), dtype=bool)
    for k in range(len(heads)):
        mA, mB, sT, cT = heads[k, 5], heads[k, 6], heads[k, 9], heads[k, 10]
        if not (np.isfinite(heads[k]).all() and np.isfinite(segs[k]).all()):
            continue
        out[k] = bool(mB > mA and 0.0 <= sT <= 1.0 and 0.0 < cT <= 1.0 and abs(((sT * sT) + (cT * cT)) - 1.0) <= TURN)
    return out


# ------------------------------------------------------------------ per row and span
def _frame(X, head):
    """(m, t, w) float64 [n] of float32 rows in a span's frame, as in the clearance rule"""
    px, py, pz = (X[:, i].astype(np.float64) for i in range(3))
    cx, cy, cz, ux, uy = head[:5]
    dx, dy, w = px - cx, py - cy, pz - cz
    return (dx * ux) + (dy * uy), (dy * ux) - (dx * uy), w


def _turn(m, t, w, head):
    """(s, e) float64 [n]: the sine of the turn the rule picks for every row, and e = 1 - cosine"""
    mA, mB, zA, kap, sT, cT = head[5:11]
    mh = np.where(m < mA, mA, m)
    mh = np.where(mh > mB, mB, mh)
    bb = (zA + ((mh - mA) * kap)) - w
    inside = (bb > 0) & ((np.abs(t) * cT) <= (bb * sT))
    rho = np.sqrt((t * t) + (bb * bb))
    s = np.where(inside, t / rho, np.where(t >= 0, sT, -sT))
    c = np.where(inside, bb / rho, cT)
    return s, 1.0 - c


def span_swing(X, heads, segs):
    """(g float64 [K,n], s float64 [K,n]): the rule's smallest d of every row to every span and the sine it is taken at
    (NaN / inf as IEEE arithmetic gives them), rows in float32 as the kernel reads them; spans that take no part have
    +inf.  One loop per span and segment."""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    heads, segs = np.asarray(heads, dtype=np.float64), np.asarray(segs, dtype=np.float64)
    K, S = segs.shape[0], segs.shape[1]
    part = takes_part(heads, segs)
    gout, sout = np.full((K, len(X)), np.inf), np.full((K, len(X)), np.nan)
    with np.errstate(all="ignore"):
        for k in range(K):
            if not part[k]:
                continue
            m, t, w = _frame(X, heads[k])
            s, e = _turn(m, t, w, heads[k])
            g = np.full(len(X), np.inf)
            for j in range(S):
                mj, zj, fj, dm, dz, df = segs[k, j]
                py, pw, ey, ez = fj * s, zj + (fj * e), df * s, dz + (df * e)
                rm, rt, rw = m - mj, t - py, w - pw
                len2 = ((dm * dm) + (ey * ey)) + (ez * ez)
                pos = len2 > 0
                q = np.where(pos, (((rm * dm) + (rt * ey)) + (rw * ez)) / np.where(pos, len2, 1.0), 0.0)
                q = np.where(q < 0, 0.0, q)
                q = np.where(q > 1, 1.0, q)
                vm, vt, vw = rm - (q * dm), rt - (q * ey), rw - (q * ez)
                d = ((vm * vm) + (vt * vt)) + (vw * vw)
                g = np.where(d < g, d, g)
            gout[k], sout[k] = g, s
    return gout, sout


def table_of(best, who, K, l2):
    """the per-span outputs over the rows with who == k, one loop per span"""
    count = np.zeros(K, dtype=np.int64)
    viol = np.zeros(K, dtype=np.int64)
    mind = np.full(K, np.inf)
    minrow = np.full(K, -1, dtype=np.int64)
    for k in range(K):
        rows = np.flatnonzero(who == k)
        count[k] = len(rows)
        viol[k] = int((best[rows] <= l2).sum())
        if len(rows):
            mind[k] = best[rows].min()
            minrow[k] = rows[best[rows] == mind[k]][0]
    return dict(count=count, violations=viol, min_dist2=mind, min_row=minrow)


def swing_reference(X, heads, segs, radius, limit, skip=None, gs=None):
    """dict of OUTPUTS: spans in ascending k, ``if g <= r2 and g < best``; ``gs``: a precomputed ``span_swing``"""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    K, n = np.asarray(segs).shape[0], len(X)
    r2, l2 = float(radius) * float(radius), float(limit) * float(limit)
    g, s = span_swing(X, heads, segs) if gs is None else gs
    alive = np.ones(n, dtype=bool) if skip is None else np.asarray(skip).reshape(-1) == 0
    best = np.full(n, np.inf)
    who = np.full(n, -1, dtype=np.int32)
    sin = np.full(n, np.nan)
    with np.errstate(invalid="ignore"):
        for k in range(K):
            take = alive & (g[k] <= r2) & (g[k] < best)
            best = np.where(take, g[k], best)
            who = np.where(take, np.int32(k), who)
            sin = np.where(take, s[k], sin)
    out = dict(dist2=best, span=who, sin=sin)
    out.update(table_of(best, who, K, l2))
    return out


# ------------------------------------------------------------------ a second, vectorised statement
def swing_by_argmin(X, heads, segs, radius, limit, skip=None):
    """dict of OUTPUTS: per span the d of all rows to all segments as [n,S] arrays and their minimum along the
    segments; the winner is the argmin over the spans within r2 - np.argmin returns the first, i.e. the lowest index
    on a tie"""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    heads, segs = np.asarray(heads, dtype=np.float64), np.asarray(segs, dtype=np.float64)
    K, n = segs.shape[0], len(X)
    r2, l2 = float(radius) * float(radius), float(limit) * float(limit)
    part = takes_part(heads, segs)
    alive = np.ones(n, dtype=bool) if skip is None else np.asarray(skip).reshape(-1) == 0
    g, sv = np.full((K, n), np.inf), np.full((K, n), np.nan)
    with np.errstate(all="ignore"):
        for k in np.flatnonzero(part):
            m, t, w = _frame(X, heads[k])
            s, e = _turn(m, t, w, heads[k])
            mj, zj, fj, dm, dz, df = (segs[k, None, :, i] for i in range(6))
            s2, e2 = s[:, None], e[:, None]
            ey, ez = df * s2, dz + (df * e2)
            rm, rt, rw = m[:, None] - mj, t[:, None] - (fj * s2), w[:, None] - (zj + (fj * e2))
            len2 = ((dm * dm) + (ey * ey)) + (ez * ez)
            num = ((rm * dm) + (rt * ey)) + (rw * ez)
            q = np.zeros_like(num)
            np.divide(num, len2, out=q, where=len2 > 0)
            q = np.where(q > 1, 1.0, np.where(q < 0, 0.0, q))
            vm, vt, vw = rm - (q * dm), rt - (q * ey), rw - (q * ez)
            d = ((vm * vm) + (vt * vt)) + (vw * vw)
            g[k] = np.where(np.isnan(d), np.inf, d).min(axis=1)              # `d < g` never takes a NaN
            sv[k] = s
        masked = np.where(alive[None, :] & (g <= r2), g, np.inf)
    if K == 0:
        best, who, sin = np.full(n, np.inf), np.full(n, -1, dtype=np.int32), np.full(n, np.nan)
    else:
        idx = np.argmin(masked, axis=0)
        best = masked[idx, np.arange(n)]
        found = best < np.inf
        who = np.where(found, idx, -1).astype(np.int32)
        sin = np.where(found, sv[idx, np.arange(n)], np.nan)
    out = dict(dist2=best, span=who, sin=sin)
    out.update(table_of(best, who, K, l2))
    return out


# ------------------------------------------------------------------ dense angles
BRUTE_ANGLES = 2001


def swing_brute(X, head, segs_k, angles=BRUTE_ANGLES, batch=87):
    """float64 [n]: the smallest distance (metres) of the rows to span k's polyline over ``angles`` equally spaced
    turns in [-Theta, Theta] - every angle for every row, the polyline distance the rule measures with"""
    X = np.asarray(X, dtype=np.float32).reshape(-1, 3)
    m, t, w = _frame(X, head)
    theta = float(np.arctan2(head[9], head[10]))
    mj, zj, fj, dm, dz, df = (segs_k[None, None, :, i] for i in range(6))
    out = np.full(len(X), np.inf)
    grid = np.linspace(-theta, theta, angles)
    for i in range(0, angles, batch):
        a = grid[i:i + batch][:, None, None]
        s, e = np.sin(a), 1.0 - np.cos(a)
        ey, ez = df * s, dz + df * e
        rm, rt, rw = m[None, :, None] - mj, t[None, :, None] - fj * s, w[None, :, None] - (zj + fj * e)
        len2 = dm * dm + ey * ey + ez * ez
        q = np.clip((rm * dm + rt * ey + rw * ez) / np.where(len2 > 0, len2, 1.0), 0.0, 1.0)
        d = (rm - q * dm) ** 2 + (rt - q * ey) ** 2 + (rw - q * ez) ** 2
        out = np.minimum(out, d.min(axis=(0, 2)))
    return np.sqrt(out)


# ------------------------------------------------------------------ the rule's boundaries on dyadic values
B_RADIUS, B_LIMIT, B_SEGMENTS = 10.0, 6.0, 4
B_SIN = float(np.round(np.sqrt(0.5) * 2.0 ** 26) / 2.0 ** 26)      # sT == cT: |t|*cT == bb*sT iff |t| == bb
NOPART = 4                                                         # the spans in front that take no part


def level_case():
    """(heads [7,11], segs [7,4,6]): the wire z = m*m/64 over m in [-32, 32] along x at y = 0 - vertices (-32, 16),
    (-16, 4), (0, 0), (16, 4), (32, 16), chord at z = 16, sag 16 - with sT = cT = B_SIN (45 degrees to 27 bits,
    sT*sT + cT*cT = 1 - 7e-9).  Spans 0..3 are that wire and take no part - a NaN among the segments, mB == mA, cT == 0,
    sT*sT + cT*cT off by 1e-5 -; span 4 is the wire, span 5 the same wire again (a tie), span 6 the wire at y = 64 with
    sT = 0, cT = 1."""
    one = cc.curve(c=1.0 / 64.0, m0=-32.0, m1=32.0)
    far = cc.curve(cy=64.0, c=1.0 / 64.0, m0=-32.0, m1=32.0)
    curves = np.stack([one] * 6 + [far])
    heads = heads_reference(curves, 45.0)
    heads[:, 9:11] = B_SIN
    segs = segments_reference(curves, B_SEGMENTS)
    assert segs[4, :, :3].tolist() == [[-32.0, 16.0, 0.0], [-16.0, 4.0, 12.0], [0.0, 0.0, 16.0], [16.0, 4.0, 12.0]]
    assert heads[4, 5:9].tolist() == [-32.0, 32.0, 16.0, 0.0]
    segs[0, 2, 5] = np.nan
    heads[1, 6] = heads[1, 5]
    heads[2, 9:11] = (1.0, 0.0)
    heads[3, 9:11] = np.sqrt((1.0 + 1e-5) / 2.0)
    heads[6, 9:11] = (0.0, 1.0)
    assert takes_part(heads, segs).tolist() == [False] * NOPART + [True] * 3
    return heads, segs


def boundary_rows():
    """(X float32 [20,3], skip uint8 [20]) for ``level_case`` at B_RADIUS, B_LIMIT"""
    f32 = np.float32
    below = lambda v: np.nextafter(f32(v), f32(-np.inf))
    above = lambda v: np.nextafter(f32(v), f32(np.inf))
    X = np.array([[0.0, 0.0, -10.0],           # 0: straight below the low point, t = 0: s = 0, g == r2 = 100: inside
                  [0.0, 0.0, below(-10.0)],    # 1: the next float32 further down: outside
                  [0.0, 0.0, -6.0],            # 2: g == l2 = 36: a violation
                  [0.0, 0.0, below(-6.0)],     # 3: the next one: within the radius, no violation
                  [0.0, 8.0, 8.0],             # 4: bb = 8 == |t|: on the sector's edge, inside it: s = 8/sqrt(128)
                  [0.0, above(8.0), 8.0],      # 5: just outside the sector: s = sT
                  [0.0, below(8.0), 8.0],      # 6: just inside
                  [0.0, -8.0, 8.0],            # 7: the other side: s = -8/sqrt(128)
                  [0.0, below(-8.0), 8.0],     # 8: just outside on that side: s = -sT
                  [0.0, above(-8.0), 8.0],     # 9: just inside
                  [30.0, 2.0, 16.0],           # 10: bb == 0: not in the sector: s = sT
                  [30.0, 2.0, below(16.0)],    # 11: bb = 2^-19 > 0 and |t|*cT > bb*sT: still s = sT
                  [30.0, 0.0, 18.0],           # 12: t == +0 above the chord: s = +sT
                  [30.0, -0.0, 18.0],          # 13: t == -0: t >= 0 holds: s = +sT
                  [np.inf, 0.0, 0.0], [0.0, -np.inf, 0.0], [0.0, 0.0, np.nan],     # 14..16
                  [0.0, 0.0, -6.0],            # 17: skipped
                  [0.0, 60.0, 3.0],            # 18: 4 m beside span 6 only, which does not swing: s = -sT = -0
                  [40.0, 3.0, 13.0]],          # 19: beyond the end: mh = 32, bb = 3 == |t|: s = 3/sqrt(18)
                 dtype=np.float32)
    skip = np.zeros(len(X), dtype=np.uint8)
    skip[17] = 1
    return X, skip


BOUNDARY_SPAN = (4, -1, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, -1, -1, -1, -1, 6, 4)     # the tie goes to span 4


# ------------------------------------------------------------------ random sloped spans
def random_case(n, K, seed, shift=None, spread=120.0, max_angle=80.0):
    """(X float32 [n,3], curves float64 [K,10], angle_deg float64 [K]): K random sagging, sloped spans in a square of
    ``spread`` metres with swing angles from 0 to ``max_angle`` degrees (one in eight exactly 0) and n rows, seven in
    ten of them scattered around a span (beyond its ends, beside, above and below it), the others anywhere"""
    rng = np.random.default_rng(seed)
    ang = rng.uniform(-0.5 * np.pi, 0.5 * np.pi, K)
    half = rng.uniform(10.0, 35.0, K)
    C = np.stack([rng.uniform(0.0, spread, K), rng.uniform(0.0, spread, K), rng.uniform(15.0, 30.0, K), np.cos(ang),
                  np.sin(ang), rng.uniform(-0.5, 0.5, K), rng.uniform(-0.1, 0.1, K), rng.uniform(0.0, 0.01, K),
                  -half * rng.uniform(0.8, 1.0, K), half], axis=1).reshape(K, 10)
    deg = np.where(rng.uniform(0.0, 1.0, K) < 0.125, 0.0, rng.uniform(0.0, max_angle, K))
    X = np.concatenate([rng.uniform(-20.0, spread + 20.0, (n, 2)), rng.uniform(0.0, 40.0, (n, 1))], axis=1)
    if K:
        k = rng.integers(0, K, n)
        m = rng.uniform(C[k, 8] - 15.0, C[k, 9] + 15.0)
        t = rng.normal(0.0, 8.0, n)
        z = C[k, 2] + C[k, 5] + m * (C[k, 6] + C[k, 7] * m) - rng.uniform(-6.0, 14.0, n)
        near = np.stack([C[k, 0] + m * C[k, 3] - t * C[k, 4], C[k, 1] + m * C[k, 4] + t * C[k, 3], z], axis=1)
        X = np.where((rng.uniform(0.0, 1.0, n) < 0.7)[:, None], near, X)
    if shift is not None:
        X = X + shift
        C[:, 0:3] += shift
    return X.astype(np.float32), C, deg


# ------------------------------------------------------------------ the scene: the line, its trees, four objects
# The pieces of section 5e's scene are cut 9 m from the towers and sag 1.2 to 1.5 m below their own chords: at 45 degrees
# their low points move 0.9 to 1.1 m sideways.  The column stands 14 m beside the line's axis at mid-span of the first
# span, 8 m from the outer conductor at rest and about 7.1 m from it at 45 degrees; the limit is set between the two.
ANGLE, RADIUS, LIMIT, SEGMENTS = 45.0, 10.0, 7.5, cc.SEGMENTS
COLUMN = (40.0, -14.0, 2.0, 22.0, 0.25)            # station, lateral, lowest and highest row, step
_SCENE = {}
_REF = {}


def _wire_z(span, station):
    s0, s1 = sp.LINE_STATIONS[span], sp.LINE_STATIONS[span + 1]
    z0, z1 = sp.LINE_BASES[span] + 21.0, sp.LINE_BASES[span + 1] + 21.0
    tau = (station - s0) / (s1 - s0)
    return z0 + (z1 - z0) * tau - 4.0 * sp.LINE_SAGS[span] * tau * (1.0 - tau)


def _chord_z(span, station, cut=9.0):
    """the height of the chord of the piece the towers' cut leaves of a conductor"""
    s0, s1 = sp.LINE_STATIONS[span] + cut, sp.LINE_STATIONS[span + 1] - cut
    return _wire_z(span, s0) + (_wire_z(span, s1) - _wire_z(span, s0)) * (station - s0) / (s1 - s0)


def wind_scene():
    """(X float32 [n,3], kind int8): ``clearance_cases.tree_scene`` (kinds 0..12) followed by a column of rows every
    0.25 m from z = 2 to z = 22, 14 m beside the axis at station 40 with 0.05 m of jitter in x and y (kind 20): clear of
    LIMIT at rest, inside it at 45 degrees; a row 3.5 m beside and 3.5 m above the chord of an outer conductor of the
    second span (kind 21): above the chord, so the wire meets it at the end of its sector; a row 5 m straight below
    the middle conductor of the second span (kind 22): nearest at angle 0; and a row 3 m beyond the end of a piece of
    the first span, 6 m beside it (kind 23): its station is clamped to the piece's end."""
    if not _SCENE:
        X, kind = cc.tree_scene()
        rng = np.random.default_rng(71)
        station, lateral, low, high, step = COLUMN
        up = np.arange(low, high + 1e-9, step)
        xy = sp._line_xy(np.full(len(up), station), np.full(len(up), lateral)) + rng.uniform(-0.05, 0.05, (len(up), 2))
        column = np.concatenate([xy, up[:, None]], axis=1)
        above = np.concatenate([sp._line_xy(np.array([115.0]), np.array([9.5])), [[_chord_z(1, 115.0) + 3.5]]], axis=1)
        under = np.concatenate([sp._line_xy(np.array([100.0]), np.array([0.0])), [[_wire_z(1, 100.0) - 5.0]]], axis=1)
        beyond = np.concatenate([sp._line_xy(np.array([76.5]), np.array([12.0])), [[22.0]]], axis=1)
        parts = [X, column.astype(np.float32), above.astype(np.float32), under.astype(np.float32),
                 beyond.astype(np.float32)]
        kinds = [kind, np.full(len(up), 20, dtype=np.int8)] + [np.full(1, v, dtype=np.int8) for v in (21, 22, 23)]
        X, kind = np.vstack(parts), np.concatenate(kinds)
        for a in (X, kind):
            a.setflags(write=False)
        _SCENE["case"] = (X, kind)
    return _SCENE["case"]


def reference():
    """the scene's reference answers, computed once: clearance_cases' ``spans`` / ``idx`` / ``curves`` / ``chord`` /
    ``tol``, ``heads`` and ``segs`` at ANGLE and SEGMENTS, ``skip``, ``gs`` (``span_swing``), the outputs of
    ``swing_reference`` at RADIUS and LIMIT, and ``rest``: ``clearance_cases.clearance_reference`` on the same rows at
    the same radius and limit.  The scene's margins are asserted here, on the host, so that the pipeline's counts,
    spans and rows may be compared exactly."""
    if not _REF:
        X, kind = wind_scene()
        r = cc.reference()
        n0 = len(cc.tree_scene()[0])
        assert np.array_equal(X[:n0], cc.tree_scene()[0])
        # the wire rule looks 2 m around a row: no new row lies that close to a row of tree_scene, so the all-pairs mask
        # of the scene is clearance_cases' followed by the new rows' own - a vertical column and single rows are no wire
        new = X[n0:].astype(np.float64)
        gap = min(float(np.sqrt(((new[:, None, :] - X[None, i:min(i + 2048, n0), :]) ** 2).sum(2).min()))
                  for i in range(0, n0, 2048))
        assert gap > 2.0 * sc.SCENE_RULE["radius"], gap
        assert not sc.drop_mask_reference(X[n0:], **sc.SCENE_RULE)[0].any()
        tw = sp.line_towers()
        near = (((X[n0:, None, :2].astype(np.float64) - tw[None, :, :2]) ** 2).sum(2) <= 9.0 * 9.0).any(axis=1)
        assert not near.any()
        skip = np.concatenate([r["skip"], np.zeros(len(X) - n0, dtype=np.uint8)])
        curves = r["curves"]
        heads, segs = heads_reference(curves, ANGLE), segments_reference(curves, SEGMENTS)
        assert np.array_equal(segs[:, :, :2], r["segs"][:, :, :2])            # the clearance rule's vertices
        gs = span_swing(X, heads, segs)
        out = swing_reference(X, heads, segs, RADIUS, LIMIT, skip=skip, gs=gs)
        rest = cc.clearance_reference(X, curves, r["segs"], RADIUS, LIMIT, skip=skip)
        tol = r["tol"]
        assert tol < 2e-5, tol
        alive = skip == 0
        dist = np.sqrt(gs[0][:, alive])
        assert np.abs(dist - RADIUS).min() > 10.0 * tol and np.abs(dist - LIMIT).min() > 10.0 * tol
        two = np.sort(dist, axis=0)[:2]
        assert (two[1] - two[0])[two[0] <= RADIUS].min() > 10.0 * tol
        for k in np.flatnonzero(out["count"] > 1):
            d = np.sort(np.sqrt(out["dist2"][out["span"] == k]))
            assert d[1] - d[0] > 10.0 * tol, k
        drest = np.sqrt(cc.span_distances(X, curves, r["segs"])[:, alive])
        assert np.abs(drest - RADIUS).min() > 10.0 * tol and np.abs(drest - LIMIT).min() > 10.0 * tol
        _REF.update(out, spans=r["spans"], idx=r["idx"], curves=curves, heads=heads, segs=segs, chord=r["chord"],
                    skip=skip, gs=gs, tol=tol, kind=kind, rest=rest)
    return _REF
