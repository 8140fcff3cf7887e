"""CPU suite: the eps-boundary fixtures of tests/dbscan_cases.py are what they claim to be.  The three restatements
of the oracle agree on them, the outcome changes between ``e`` and its predecessor ``em``, a float32-only predicate
gets them wrong, and scikit-learn's own output for the lattices is pinned."""
import hashlib
import math
import os

import numpy as np
import pytest

import dbscan_cases as dc
from oracle import dbscan as odb

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PY_ORACLE_ROWS = 2000        # the literal python restatements walk every neighbour list of every core point (minutes
                             # for thousands of core points with thousands of neighbours each): above this size only
                             # the tile lattice goes through them, at the min_samples that leaves few core points.  For
                             # the others the core mask is compared with the counts of D, and the labels with sklearn's
PY_ORACLE_PICKS = 4          # ... and of the 32 k-distance picks of a combination the first 4; the C one takes all


def _agree(X, eps, ms, python=True):
    lab, core = odb.dbscan_fit_c(X, eps, ms)
    if python:
        for f in (odb.dbscan_rule, odb.dbscan_fit_numpy):
            l2, c2 = f(X, eps, ms)
            np.testing.assert_array_equal(l2, lab)
            np.testing.assert_array_equal(c2, core)
    return lab, core


def _k(lab):
    return int(lab.max()) + 1


# ------------------------------------------------------------------ a. lattices
@pytest.mark.parametrize("name", sorted(dc.LATTICES))
def test_lattice_is_on_the_boundary(oracle_clib, name):
    X, eps, em, mss, p = dc.lattice_case(name)
    ce, cm, cs = dc.neighbour_counts(X, [eps, em]).tolist() + dc.neighbour_counts(X, [eps], strict=True).tolist()
    ce, cm, cs = np.asarray(ce), np.asarray(cm), np.asarray(cs)
    np.testing.assert_array_equal(cm, cs)                 # nextafter(eps, 0) drops exactly the pairs at d2 == eps*eps
    assert ce[p] > cm[p] and mss == [ce[p], ce[p] + 1, cm[p] + 1]
    assert sorted(np.random.default_rng(0).permutation(len(X)).tolist()) != X[:, 0].argsort(kind="stable").tolist()
    for ms in mss:
        py = len(X) <= PY_ORACLE_ROWS or (name == "tile" and ms == mss[2])
        le, core_e = _agree(X, eps, ms, py)
        lm, core_m = _agree(X, em, ms, py)
        np.testing.assert_array_equal(core_e, (ce >= ms).astype(np.uint8))
        np.testing.assert_array_equal(core_m, (cm >= ms).astype(np.uint8))     # '<' for '<=' in D
        if ms == mss[0]:
            assert core_e[p] and not core_m[p]
        elif ms == mss[1]:
            assert not core_e[p] and not core_m[p]
        else:
            assert core_e[p] and not core_m[p]
            assert (core_e != core_m).any() and (cs >= ms)[p] == 0
    # the branch of db_core_k the fixture is built for, with boundary pairs in it
    cnt, tot = dc.cell_census(X, eps)
    hang = (ce >= mss[2]) & (cm < mss[2])                 # core status hangs on the sphere points
    if name == "few":
        assert cnt.max() < 24 and hang.any()
    elif name == "tile":
        assert (hang & (cnt >= 24) & (cnt < mss[2])).any() and tot.max() < 8192
    elif name == "long":
        assert (hang & (cnt < 24) & (tot >= 8192)).any() and (hang & (cnt >= 24) & (tot >= 8192)).any()
        assert cnt.max() < mss[2]
    else:
        assert (cnt >= mss[0] + 1).any() and (hang & (cnt < 24)).any() and (cnt[hang] < mss[2]).all()


def _lattice_sha(X):
    return hashlib.sha256(np.ascontiguousarray(X).tobytes()).hexdigest()


def test_lattice_golden_holds_sklearn_output_for_every_lattice():
    g = np.load(os.path.join(GOLD, "dbscan_lattice_ties.npz"))
    assert sorted(str(s) for s in g["names"]) == sorted(dc.LATTICES)      # the ball tree agreed on all of them


@pytest.mark.parametrize("name", sorted(dc.LATTICES))
def test_dbscan_c_oracle_matches_sklearn_on_lattice_ties(oracle_clib, name):
    g = np.load(os.path.join(GOLD, "dbscan_lattice_ties.npz"))
    X, eps, em, mss, p = dc.lattice_case(name)
    assert _lattice_sha(X) == str(g[f"{name}_sha"]), "seeded lattice differs from the fixture's"
    assert mss == g[f"{name}_min_samples"].tolist() and eps == float(g[f"{name}_eps"])
    for i, ms in enumerate(mss):
        for j, e in enumerate((eps, em)):
            lab, core = odb.dbscan_fit_c(X, e, ms)
            np.testing.assert_array_equal(lab, g[f"{name}_labels"][i, j])
            np.testing.assert_array_equal(core, g[f"{name}_core"][i, j])


def test_lattice_ties_vs_live_sklearn(oracle_clib):
    pytest.importorskip("sklearn")
    X, eps, em, mss, p = dc.lattice_case("few")
    for ms in mss:
        for e in (eps, em):
            ref, rcore = odb.dbscan_fit_sklearn(X, e, ms)
            lab, core = odb.dbscan_fit_c(X, e, ms)
            np.testing.assert_array_equal(lab, ref)
            np.testing.assert_array_equal(core, rcore)


# ------------------------------------------------------------------ b. k-distance picks
_CLOUDS = {}


def _cloud(name):
    if name not in _CLOUDS:
        X = dc.KDIST_CLOUDS[name]()
        _CLOUDS[name] = (X, dc.pair_d2(X))
    return _CLOUDS[name]


@pytest.mark.parametrize("ms", dc.KDIST_MS)
@pytest.mark.parametrize("cloud", sorted(dc.KDIST_CLOUDS))
def test_kdist_picks_flip_between_e_and_em(oracle_clib, cloud, ms):
    X, D = _cloud(cloud)
    picks, skipped = dc.kdist_picks(X, D, ms)
    assert skipped <= dc.KDIST_PICKS * 5 // 100, skipped
    assert len(picks) + skipped == dc.KDIST_PICKS
    for n, (i, e, em, j) in enumerate(picks):
        le, ce = _agree(X, e, ms, n < PY_ORACLE_PICKS)
        lm, cm = _agree(X, em, ms, n < PY_ORACLE_PICKS)
        if ms == 1:
            assert ce.all() and cm.all() and le[i] == le[j] and lm[i] != lm[j], (i, j)
            assert _k(lm) == _k(le) + 1
            assert dc.f32_only_within(X[i], X[j], e) == dc.f32_only_within(X[i], X[j], em)
        else:
            assert ce[i] == 1 and cm[i] == 0, i
            fe, fm = dc.f32_only_core(X, e, ms), dc.f32_only_core(X, em, ms)
            assert fe[i] == fm[i] and (fe[i] != ce[i] or fm[i] != cm[i])


def test_tight_cloud_needs_the_full_guard_band():
    """the picks of the tight cloud are decided rightly behind a 2^-20 guard band and wrongly, somewhere, behind a
    2^-24 one: float32 distances there are off by more than one ulp"""
    X, D = _cloud("tight")
    wrong = 0
    for ms in dc.KDIST_MS:
        for i, e, em, j in dc.kdist_picks(X, D, ms)[0]:
            for eps in (e, em):
                got, want = dc.banded_count(X, i, eps, 2.0 ** -20)
                assert got == want, (ms, i)
                got, want = dc.banded_count(X, i, eps, 2.0 ** -24)
                wrong += got != want
    assert wrong >= 3, wrong


# ------------------------------------------------------------------ c. link at the boundary
@pytest.mark.parametrize("epsg", [False, True], ids=["local", "epsg"])
@pytest.mark.parametrize("halo", [False, True], ids=["clumps", "halo"])
@pytest.mark.parametrize("direction", sorted(dc.DIRECTIONS))
def test_link_hangs_on_one_pair(oracle_clib, direction, halo, epsg):
    X, ms, e, em, (a, b) = dc.link_case(direction, halo, epsg)
    le, ce = _agree(X, e, ms)
    lm, cm = _agree(X, em, ms)
    for core in (ce, cm):
        assert core[a].all() and core[b].all()
    np.testing.assert_array_equal(ce, cm)
    assert _k(le) == 1 and _k(lm) == 2 and len(set(lm[a])) == 1 and len(set(lm[b])) == 1
    D = dc.pair_d2(X[b], X[a])
    ia, ib = np.unravel_index(np.argmin(D), D.shape)
    assert (D <= em * em).sum() == 0 and (D <= e * e).sum() >= 1      # the pairs at d2* make the link, no other
    assert dc.f32_only_within(X[a[ia]], X[b[ib]], e) == dc.f32_only_within(X[a[ia]], X[b[ib]], em)
    cnt, _ = dc.cell_census(X, e)
    if halo:
        assert cnt.max() < ms                                         # no dense cell: the sweeping union kernels decide
    else:
        assert cnt.max() >= ms


# ------------------------------------------------------------------ d. border at the boundary
@pytest.mark.parametrize("two,epsg", [(False, False), (False, True), (True, False)], ids=["one", "one-epsg", "two"])
def test_border_hangs_on_one_pair(oracle_clib, two, epsg):
    X, ms, e, em, lone, a, *rest = dc.border_case(two, epsg)
    le, ce = _agree(X, e, ms)
    lm, cm = _agree(X, em, ms)
    np.testing.assert_array_equal(ce, cm)
    assert ce[a].all() and not ce[lone] and (le[a] == 0).all()
    assert le[lone] == 0 and lm[lone] == -1                           # the smallest id wins at e, noise at em
    D = dc.pair_d2(X[a], X[lone])[0]
    assert (D <= e * e).sum() == 1
    near = a[int(np.argmin(D))]
    assert dc.f32_only_within(X[lone], X[near], e) == dc.f32_only_within(X[lone], X[near], em)
    if two:
        b = rest[0]
        assert ce[b].all() and (le[b] == 1).all() and _k(le) == 2
        assert (dc.pair_d2(X[b], X[lone])[0] <= e * e).sum() == 1


# ------------------------------------------------------------------ the all-pairs statements themselves
def test_relabel_and_first_rows_references_on_the_tie_fixture():
    a = np.column_stack([np.linspace(0, 1, 30), np.zeros(30), np.zeros(30)])
    b = np.column_stack([np.linspace(3.2, 4.2, 30), np.zeros(30), np.zeros(30)])
    X = np.vstack([b, [[2.1, 0, 0]], a]).astype(np.float32)
    lab, core = odb.dbscan_fit_numpy(X, 1.15, 8)
    assert dc.first_core_rows_reference(core, lab, 2).tolist() == [0, 31]
    np.testing.assert_array_equal(dc.relabel_reference(X, core, lab, [0, 1], 1.15), lab)
    sw = dc.relabel_reference(X, core, lab, [1, 0], 1.15)
    assert (sw[:30] == 1).all() and (sw[31:] == 0).all() and sw[30] == 0
    dr = dc.relabel_reference(X, core, sw, [5], 1.15)                  # shorter than the ids in use: id 1 is dropped
    assert (dr[:30] == -1).all() and (dr[31:] == 5).all() and dr[30] == 5
    ch = dc.relabel_reference(X, core, lab, [0, 1], 1.15, chunk_size=31)
    assert ch[30] == 0 and (ch == lab).all()
    ch = dc.relabel_reference(X, core, lab, [-1, 1], 1.15, chunk_size=31)
    assert ch[30] == -1                                                # cluster 1's core rows lie in the other chunk
