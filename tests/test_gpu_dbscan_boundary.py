"""Stage C on the eps boundary, and its continuation calls against all pairs.

Every input comes from tests/dbscan_cases.py: pairs exactly at eps (lattices), eps set to the double at which one
row's k-th neighbour enters (k-distance picks), a link and a border that hang on one pair.  Each runs at ``e`` and at
its predecessor ``em`` through every host path of dbscan_run and must equal the all-pairs C oracle exactly.  The
continuation calls (relabel, first_core_rows, strip_pairs) are compared with the all-pairs statements of that module."""
import math

import numpy as np
import pytest
import torch

import dbscan_cases as dc
from oracle import dbscan as odb
from pointcloudhookup_amd import _lib, ops

pytestmark = pytest.mark.gpu

ROW_TABLE = 65536            # cells the neighbour-row table holds for n >= 65536 rows (max(n/4, 65536))


# ------------------------------------------------------------------ running and comparing
def _fit(X, cuda, eps, ms, chunk=0, mode="auto", aabb=None):
    try:
        ops.set_dbscan_sort_mode(mode)
        lab, core, k = ops.dbscan(torch.from_numpy(np.ascontiguousarray(X)).to(cuda), eps, ms, chunk, aabb=aabb,
                                  want_core=True)
    finally:
        ops.set_dbscan_sort_mode("auto")
    return lab.cpu().numpy(), core.cpu().numpy(), k


def _ref(X, eps, ms, chunk=0):
    """labels of the chunked reference, the core mask of its fits, the cluster count"""
    lab = odb.dbscan_chunked(X, eps, ms, chunk, fit="c")
    cs = chunk if chunk > 0 else len(X)
    core = np.concatenate([odb.dbscan_fit_c(X[s:s + cs], eps, ms)[1] for s in range(0, len(X), cs)])
    return lab, core, (int(lab.max()) + 1 if (lab >= 0).any() else 0)


def _same(got, want, what):
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"core mask, {what}")
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"labels, {what}")
    assert got[2] == want[2], what


def _isolated(count, eps, corner):
    """count rows no two of which (nor any fixture row below ``corner``) are within eps: a lattice of 4 eps steps"""
    side = int(math.ceil(count ** (1.0 / 3.0)))
    g = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:count]
    step = max(4.0 * eps, 2.0)
    return (np.asarray(corner, dtype=np.float64) + step * (g + 3)).astype(np.float32)


def _rowless(X, eps, chunk):
    """X in front of the second chunk of a call with more cells than the row table holds: the other rows are
    isolated, one cell each.  Returns (rows, slice of X in them)."""
    nchunks = -(-(ROW_TABLE + 4096 + len(X)) // chunk)
    pad = _isolated(nchunks * chunk - len(X), eps, X.max(0))
    rows = np.vstack([pad[:chunk], X, pad[chunk:]])
    assert len(rows) >= ROW_TABLE and dc.count_cells(rows, eps, chunk) > max(ROW_TABLE, len(rows) // 4)
    return rows, slice(chunk, chunk + len(X))


def _far(X):
    """one extra row at ~1e30: the cell key no longer fits 64 bits (compressed coordinates, or per-chunk refits)"""
    return np.vstack([X, np.array([[1e30, -1e30, 1e29]], np.float32)])


def _boxes(X, eps):
    """the exact box, a superset that moves the grid origin, and two origins a whole number of cells (up to float32
    rounding) below the lower corner, so that the rows of the lower faces fall on cell faces"""
    lo, hi = X.min(0).astype(np.float64), X.max(0).astype(np.float64)
    cell = eps / math.sqrt(3.0) * (1.0 - 1.0 / 65536.0)
    out = {"exact": np.concatenate([lo, hi]),
           "superset": np.concatenate([lo - eps * np.array([0.37, 1.11, 2.73]), hi + eps * np.array([1.9, 0.2, 0.6])])}
    for name, k in (("cells-1-2-3", np.array([1.0, 2.0, 3.0])), ("cells-4-1-2", np.array([4.0, 1.0, 2.0]))):
        out[name] = np.concatenate([(lo - k * cell).astype(np.float32).astype(np.float64), hi + eps])
    return {k: v.astype(np.float32) for k, v in out.items()}


def _all_paths(X, eps, ms, cuda, what, chunks=3, rowless_chunk=0, want0=None):
    """every host path of dbscan_run on one input; returns the reference of the single fit"""
    want0 = want0 or _ref(X, eps, ms, 0)
    for mode in ("chunk", "global", "auto"):                          # the cell sorts, one fit
        _same(_fit(X, cuda, eps, ms, 0, mode), want0, f"{what} single fit sort={mode}")
    cs = -(-len(X) // chunks)
    wantc = _ref(X, eps, ms, cs)                                      # several fits: pairs across a cut do not count
    for mode in ("chunk", "global"):
        _same(_fit(X, cuda, eps, ms, cs, mode), wantc, f"{what} chunk={cs} sort={mode}")
    for name, box in _boxes(X, eps).items():                          # caller-supplied boxes: other cell boundaries
        _same(_fit(X, cuda, eps, ms, 0, "auto", box), want0, f"{what} aabb={name}")
        _same(_fit(X, cuda, eps, ms, cs, "chunk", box), wantc, f"{what} aabb={name} chunk={cs}")
    F = _far(X)
    _same(_fit(F, cuda, eps, ms, 0), _ref(F, eps, ms, 0), f"{what} compressed coordinates")
    _same(_fit(F, cuda, eps, ms, cs), _ref(F, eps, ms, cs), f"{what} per-chunk refits chunk={cs}")
    if rowless_chunk:
        R, sel = _rowless(X, eps, rowless_chunk)
        wr = _ref(R, eps, ms, rowless_chunk)
        for mode in ("chunk", "global"):
            _same(_fit(R, cuda, eps, ms, rowless_chunk, mode), wr, f"{what} no row table sort={mode}")
        if len(X) <= rowless_chunk:                                   # the isolated rows add no neighbour
            np.testing.assert_array_equal(wr[1][sel], want0[1])
    return want0


# ------------------------------------------------------------------ a. lattices
@pytest.mark.parametrize("name", sorted(dc.LATTICES))
def test_lattice_ties_on_every_host_path(cuda, oracle_clib, name):
    X, eps, em, mss, p = dc.lattice_case(name)
    for ms in mss:
        for e in (eps, em):
            rl = (20000 if name == "long" else 10000) if ms == mss[2] else 0
            want = _all_paths(X, e, ms, cuda, f"lattice {name} ms={ms} eps={e!r}", rowless_chunk=rl)
            if ms != mss[1]:
                assert want[1][p] == (1 if e == eps else 0)           # the probe is core at eps alone
            else:
                assert want[1][p] == 0


@pytest.mark.parametrize("name", sorted(dc.LATTICES))
def test_lattice_reaches_its_branch_of_db_core(cuda, oracle_clib, name):
    """the counting build of db_core_k (same control flow) shows which path the cells took"""
    X, eps, em, mss, p = dc.lattice_case(name)
    ms = mss[2]
    cnt, tot = dc.cell_census(X, eps)
    dev = torch.from_numpy(np.ascontiguousarray(X)).to(cuda)
    for e in (eps, em):
        plain = _fit(X, cuda, e, ms)
        try:
            ops.set_pair_counting(True)
            fit = ops.DbscanFit(dev, e, ms, 0)
            stats = fit.pair_stats()
        finally:
            ops.set_pair_counting(False)
        _same((fit.labels.cpu().numpy(), fit.core.cpu().numpy(), fit.nclusters), plain, f"counting fit {name}")
        _same(plain, _ref(X, e, ms), f"plain fit {name}")
        assert stats["cells_tested"] > 0 and stats["pair_tests"] > 0, stats
        if name == "few":
            assert cnt.max() < 24 and stats["tiles_staged"] == 0, stats
        elif name == "tile":
            assert stats["tiles_staged"] > 0, stats
        elif name == "long":
            assert ((cnt < 24) & (tot >= 8192)).any() and ((cnt >= 24) & (tot >= 8192)).any()
            assert stats["tiles_staged"] > 0, stats
        else:                                                          # dense cells never reach the test path
            ncell = dc.count_cells(X, e)
            dense = len(np.unique(dc.grid_cells(X, e)[cnt >= ms], axis=0))
            assert dense > 0 and stats["cells_tested"] <= ncell - dense, (stats, ncell, dense)


# ------------------------------------------------------------------ b. k-distance picks
_CLOUDS = {}


def _cloud(name):
    if name not in _CLOUDS:
        X = dc.KDIST_CLOUDS[name]()
        _CLOUDS[name] = (X, dc.pair_d2(X))
    return _CLOUDS[name]


@pytest.mark.parametrize("ms", dc.KDIST_MS)
@pytest.mark.parametrize("cloud", sorted(dc.KDIST_CLOUDS))
def test_kdist_picks_flip_on_the_gpu(cuda, oracle_clib, cloud, ms):
    X, D = _cloud(cloud)
    picks, skipped = dc.kdist_picks(X, D, ms)
    assert skipped <= dc.KDIST_PICKS * 5 // 100, skipped
    cs = -(-len(X) // 3)
    for n, (i, e, em, j) in enumerate(picks):
        got = {}
        for eps in (e, em):
            what = f"k-distance pick row {i} ms={ms} eps={eps!r}"
            want0 = _ref(X, eps, ms, 0)
            if n < 2:                                                  # every host path for the first picks ...
                _all_paths(X, eps, ms, cuda, what, rowless_chunk=10000 if (n == 0 and ms in (2, 20)) else 0,
                           want0=want0)
            else:                                                      # ... the sorts, one fit and three, for all
                wantc = _ref(X, eps, ms, cs)
                for mode in ("chunk", "global"):
                    _same(_fit(X, cuda, eps, ms, 0, mode), want0, f"{what} sort={mode}")
                    _same(_fit(X, cuda, eps, ms, cs, mode), wantc, f"{what} chunk={cs} sort={mode}")
            got[eps] = _fit(X, cuda, eps, ms, 0)
            _same(got[eps], want0, what)
        if ms == 1:
            assert got[e][0][i] == got[e][0][j] and got[em][0][i] != got[em][0][j], f"pick row {i}: link to row {j}"
        else:
            assert got[e][1][i] == 1 and got[em][1][i] == 0, f"pick row {i}: core flag does not flip"


# ------------------------------------------------------------------ c. link, d. border
@pytest.mark.parametrize("epsg", [False, True], ids=["local", "epsg"])
@pytest.mark.parametrize("halo", [False, True], ids=["clumps", "halo"])
@pytest.mark.parametrize("direction", sorted(dc.DIRECTIONS))
def test_link_at_the_boundary(cuda, oracle_clib, direction, halo, epsg):
    X, ms, e, em, (a, b) = dc.link_case(direction, halo, epsg)
    for eps, k in ((e, 1), (em, 2)):
        what = f"link {direction} halo={halo} epsg={epsg} eps={eps!r}"
        want = _all_paths(X, eps, ms, cuda, what, chunks=1, rowless_chunk=10000 if not epsg else 0)
        got = _fit(X, cuda, eps, ms, 0)
        assert want[2] == k and got[2] == k, what
        assert (got[0][a[0]] == got[0][b[0]]) == (k == 1), what


@pytest.mark.parametrize("two,epsg", [(False, False), (False, True), (True, False)], ids=["one", "one-epsg", "two"])
def test_border_at_the_boundary(cuda, oracle_clib, two, epsg):
    X, ms, e, em, lone, a, *rest = dc.border_case(two, epsg)
    for eps, lab in ((e, 0), (em, -1)):
        what = f"border two={two} epsg={epsg} eps={eps!r}"
        want = _all_paths(X, eps, ms, cuda, what, chunks=1, rowless_chunk=10000)
        got = _fit(X, cuda, eps, ms, 0)
        assert want[0][lone] == lab and got[0][lone] == lab and got[1][lone] == 0, what


def test_relabel_moves_the_lone_point_at_the_boundary(cuda, oracle_clib):
    """swapped ids: at e the lone point between the two clumps follows the smallest NEW id, at em it stays noise"""
    X, ms, e, em, lone, a, b = dc.border_case(True)
    dev = torch.from_numpy(X).to(cuda)
    for eps in (e, em):
        fit = ops.DbscanFit(dev, eps, ms, 0)
        lab0, core = fit.labels.cpu().numpy().copy(), fit.core.cpu().numpy()
        assert fit.nclusters == 2 and (lab0[a] == 0).all() and (lab0[b] == 1).all()
        assert fit.first_core_rows().cpu().tolist() == [int(a[0]), int(b[0])]
        got = fit.relabel(torch.tensor([1, 0], dtype=torch.int32, device=cuda)).cpu().numpy().copy()
        np.testing.assert_array_equal(got, dc.relabel_reference(X, core, lab0, [1, 0], eps))
        assert (got[a] == 1).all() and (got[b] == 0).all() and got[lone] == (0 if eps == e else -1)
        got2 = fit.relabel(torch.tensor([-1, 7], dtype=torch.int32, device=cuda)).cpu().numpy()
        np.testing.assert_array_equal(got2, dc.relabel_reference(X, core, got, [-1, 7], eps))
        assert got2[lone] == (7 if eps == e else -1) and (got2[b] == -1).all()


# ------------------------------------------------------------------ continuation calls against all pairs
EPS_C, MS_C = 1.0, 10


def _maps(k, seed):
    rng = np.random.default_rng(seed)
    perm = rng.permutation(k)
    drop = perm.copy()
    drop[rng.choice(k, max(1, k // 3), replace=False)] = -1
    merge = np.arange(k) // 3
    return {"identity": np.arange(k), "permutation": perm, "drop a third": drop, "several to one": merge,
            "shorter than nclusters": perm[:max(1, k - 3)] % max(1, k - 3)}


def _continuation(X, cuda, chunk, mode, what, maps=None, check_fit=True):
    dev = torch.from_numpy(np.ascontiguousarray(X)).to(cuda)

    def fit():
        try:
            ops.set_dbscan_sort_mode(mode)
            return ops.DbscanFit(dev, EPS_C, MS_C, chunk)
        finally:
            ops.set_dbscan_sort_mode("auto")

    f = fit()
    k = f.nclusters
    lab0, core = f.labels.cpu().numpy().copy(), f.core.cpu().numpy()
    if check_fit:
        _same((lab0, core, k), _ref(X, EPS_C, MS_C, chunk), what)
    assert k >= 4 and ((lab0 >= 0) & (core == 0)).any(), what         # clusters and border rows
    rows = f.first_core_rows().cpu().numpy()
    assert len(rows) == k and (np.diff(rows) > 0).all(), what
    np.testing.assert_array_equal(rows, dc.first_core_rows_reference(core, lab0, k), err_msg=what)
    all_maps = _maps(k, 5)
    for name in (maps or all_maps):
        cmap = all_maps[name]
        f = fit()                                                      # every map starts from the fit's own labels
        got = f.relabel(torch.from_numpy(cmap.astype(np.int32)).to(cuda)).cpu().numpy()
        want = dc.relabel_reference(X, core, lab0, cmap, EPS_C, chunk)
        np.testing.assert_array_equal(got, want, err_msg=f"{what} relabel {name}")
        if name == "drop a third":                                     # a second relabel maps cores by their CURRENT label
            k2 = int(cmap.max()) + 1
            second = np.random.default_rng(9).permutation(k2)
            second[0] = -1
            got2 = f.relabel(torch.from_numpy(second.astype(np.int32)).to(cuda)).cpu().numpy()
            np.testing.assert_array_equal(got2, dc.relabel_reference(X, core, want, second, EPS_C, chunk),
                                          err_msg=f"{what} two relabels in a row")
    return lab0, core, k


@pytest.mark.parametrize("mode", ["chunk", "global"])
@pytest.mark.parametrize("chunk", [0, 4000])
def test_continuation_calls_against_all_pairs(cuda, oracle_clib, chunk, mode):
    X = dc.bridge_cloud(12000, 31)
    lab, core, k = _continuation(X, cuda, chunk, mode, f"bridge cloud chunk={chunk} sort={mode}")
    if chunk == 0:                                                     # rows between two blobs touch both clusters
        border = np.flatnonzero((lab >= 0) & (core == 0))
        hit = dc.pair_d2(X[core == 1], X[border]) <= EPS_C * EPS_C
        assert max(len(set(lab[core == 1][h])) for h in hit) >= 2


def test_continuation_calls_with_compressed_coordinates(cuda, oracle_clib):
    X = _far(dc.bridge_cloud(6000, 32, epsg=False))
    _continuation(X, cuda, 0, "auto", "bridge cloud, compressed coordinates")


def test_continuation_calls_without_the_row_table(cuda, oracle_clib):
    X = dc.bridge_cloud(3000, 33)
    pad = _isolated(ROW_TABLE + 6000, EPS_C, X.max(0))
    R = np.vstack([pad[:1000], X, pad[1000:]])
    assert dc.count_cells(R, EPS_C) > max(ROW_TABLE, len(R) // 4)
    _continuation(R, cuda, 0, "global", "bridge cloud, no row table", maps=["permutation", "drop a third"],
                  check_fit=False)
    lab = _fit(R, cuda, EPS_C, MS_C, 0, "global")[0]
    np.testing.assert_array_equal(lab[1000:1000 + len(X)], _ref(X, EPS_C, MS_C)[0])     # the pad adds no neighbour


def test_strip_pairs_on_a_chunked_fit(cuda, oracle_clib):
    X = dc.bridge_cloud(12000, 31)
    chunk = 4000
    fit = ops.DbscanFit(torch.from_numpy(X).to(cuda), EPS_C, MS_C, chunk)
    lab, core = fit.labels.cpu().numpy(), fit.core.cpu().numpy()
    lo, hi = np.float32(20.0), np.float32(40.0)
    pairs, cnt = fit.strip_pairs(lo, hi, 8192)
    m = int(cnt.item())
    assert 0 < m <= 8192
    pr = pairs[:m].cpu().numpy().astype(np.int64)
    strip = (core == 1) & (X[:, 0] >= lo) & (X[:, 0] < hi)
    assert strip[pr[:, 0]].all()                                       # strip core rows ...
    np.testing.assert_array_equal(lab[pr[:, 0]], pr[:, 1])             # ... with their own label
    assert len(np.unique(pr[:, 0])) == m
    for s in range(0, len(X), chunk):                                  # per chunk: a representative of its own
        rows = s + np.flatnonzero(strip[s:s + chunk])                  # cluster within eps of every strip core row
        reps = pr[(pr[:, 0] >= s) & (pr[:, 0] < s + chunk)]
        assert len(rows) and len(reps)
        near = (dc.pair_d2(X[reps[:, 0]], X[rows]) <= EPS_C * EPS_C) & (lab[rows][:, None] == reps[None, :, 1])
        assert near.any(1).all()


def test_per_chunk_refits_refuse_the_continuation_calls(cuda, oracle_clib):
    X = _far(dc.bridge_cloud(6000, 32))
    fit = ops.DbscanFit(torch.from_numpy(X).to(cuda), EPS_C, MS_C, 2000)
    _same((fit.labels.cpu().numpy(), fit.core.cpu().numpy(), fit.nclusters), _ref(X, EPS_C, MS_C, 2000), "refits")
    before = fit.labels.clone()
    cmap = torch.zeros(fit.nclusters, dtype=torch.int32, device=cuda)
    for call in (lambda: fit.relabel(cmap), fit.first_core_rows):
        with pytest.raises(_lib.PchError, match="untouched workspace") as err:
            call()
        assert err.value.code == -1                                    # PCH_ERR_ARG
    torch.cuda.synchronize()
    assert torch.equal(fit.labels, before)
