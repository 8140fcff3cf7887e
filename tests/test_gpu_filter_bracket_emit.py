"""Height filter, percentile bracket from the centroid summary (MsBracket, pch_mean.h; sel_collect_k, pch_filter.hip).

Above 65 536 rows (where the summary has a sampled estimate: ms_predicts, pch_mean.hip) the summary pass keeps, per
1024-row block, the z values inside a bracket of the wanted percentile at the front of the block's segment plus one
small record.  Whether the bracket holds the wanted order statistics is checked on the device; if not, the select reads
the z of the rows.  A smaller cloud has no bracket: its select reads the z of the rows at once.

Every case runs ops.ground_filter on two routes and holds each against oracle.ground_filter bit for bit:
  bracket   the default
  rows      PCH_GF_BRACKET_INVALID: the bracket's device check fails, the three select passes read the rows (stride 3)
and the two must equal each other.  A route is a property of the process (the toggle is read once), so each route
is one child process that runs all cases one after the other ON ONE WORKSPACE (ops keeps a grow-only buffer): stale
per-block records and stale segment fronts of the call before are always there to be tripped over - also by the small
clouds, which lay the workspace out without segments and records.
"""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROUTES = {"bracket": {}, "rows": {"PCH_GF_BRACKET_INVALID": "1"}}

CASES = ["flat", "pct0", "pct25", "pct50", "pct100", "constant", "two_inside", "two_last_of_lower", "two_first_of_upper",
         "quantised", "ascending", "cliff", "nan_rows", "nan_block", "inf_rows", "nan_inf_mixed",
         # around one 1024-row summary block, one 16 384-row sweep tile and the largest cloud without a bracket (65 536)
         "n1", "n2", "n1023", "n1025", "n16384", "n16385", "n65536", "n65537",
         "n131072", "n131073", "n1048575", "n1048577",
         "reuse_1m_a", "reuse_small", "reuse_200k", "reuse_1m_b"]

CHILD = r'''
import hashlib, json, sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
from oracle import ground_filter as ogf
from pointcloudhookup_amd import ops

OFF = np.array([437000.0, 3139000.0, 80.0])


def flat(n, seed):
    """flat ground N(0, 0.05) with 8 % tall rows"""
    rng = np.random.default_rng(seed)
    pts = np.column_stack([rng.uniform(0, 2000, n), rng.uniform(0, 100, n), rng.normal(0, 0.05, n)])
    tall = rng.random(n) < 0.08
    pts[tall, 2] = rng.uniform(4, 40, tall.sum())
    return pts, rng


def two_values(lower):
    """n = 262 149: the 25 % rank is row 65 537 of the sorted column ((n - 1) / 4 exactly)"""
    n = 262_149
    pts, rng = flat(n, 23)
    z = np.full(n, 5.0)
    z[:lower] = 0.0
    pts[:, 2] = z[rng.permutation(n)]
    return pts


def build(case):
    pct = 25.0
    if case in ("flat", "pct0", "pct25", "pct50", "pct100"):
        pts, _ = flat(400_003, 11)
        pct = {"flat": 25.0, "pct0": 0.0, "pct25": 25.0, "pct50": 50.0, "pct100": 100.0}[case]
    elif case == "constant":
        pts, _ = flat(300_000, 12)
        pts[:, 2] = 1.5
    elif case == "two_inside":
        pts = two_values(100_000)
    elif case == "two_last_of_lower":
        pts = two_values(65_538)
    elif case == "two_first_of_upper":
        pts = two_values(65_537)
    elif case == "quantised":
        pts, _ = flat(400_003, 13)
        pts[:, 2] = np.round(pts[:, 2], 2)
    elif case == "ascending":
        pts, _ = flat(500_000, 14)
        pts[:, 2] = np.sort(pts[:, 2])
    elif case == "cliff":
        pts, rng = flat(400_003, 11)
        low = rng.random(len(pts)) < 0.2503
        pts[low, 2] = rng.uniform(-500, -400, low.sum())
    elif case in ("nan_rows", "inf_rows", "nan_inf_mixed"):
        pts, rng = flat(400_003, 15)
        rows = rng.choice(len(pts), 9, replace=False)
        vals = {"nan_rows": [np.nan] * 9, "inf_rows": [np.inf] * 9,
                "nan_inf_mixed": [np.nan, np.inf, -np.inf] * 3}[case]
        pts[rows, 2] = vals
    elif case == "nan_block":
        pts, _ = flat(200_000, 16)
        pts[2048:3072, 2] = np.nan                    # a whole block: its sampled row is NaN whichever row that is
    elif case.startswith("n"):
        pts, _ = flat(int(case[1:]), 17)
    elif case == "reuse_1m_a":
        pts, _ = flat(1_000_000, 18)
    elif case == "reuse_small":
        pts, _ = flat(40_000, 21)                     # no bracket: the rows' select on a workspace full of segments
    elif case == "reuse_200k":
        pts, _ = flat(200_000, 19)
    elif case == "reuse_1m_b":
        pts, _ = flat(1_000_000, 20)
    else:
        raise KeyError(case)
    return (pts + OFF).astype(np.float32), pct


def same_bits(a, b):
    """bit for bit; NaN only has to be NaN on both sides (payload bits aside)"""
    a, b = np.atleast_1d(np.asarray(a, np.float32)), np.atleast_1d(np.asarray(b, np.float32))
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def run(case):
    raw, pct = build(case)
    ref = ogf.ground_filter(raw, pct=pct)
    got = ops.ground_filter(torch.from_numpy(raw).cuda(), pct=pct)
    gp, gi = got["points"].cpu().numpy(), got["index"].cpu().numpy()
    f = ref["filtered"]
    bad = []
    if not same_bits(got["centroid"], ref["centroid"]): bad.append("centroid")
    if not same_bits(got["base"], ref["base"]): bad.append("base %r %r" % (got["base"], ref["base"]))
    if not same_bits(got["threshold"], ref["threshold"]): bad.append("threshold")
    if bool(got["used_fallback"]) != bool(ref["used_fallback"]): bad.append("used_fallback")
    if int(got["count"]) != len(f): bad.append("count %d %d" % (got["count"], len(f)))
    elif not same_bits(gp, f): bad.append("points")
    if not np.array_equal(gi, np.flatnonzero(ref["keep"])): bad.append("index")
    fin = np.isfinite(f).all(axis=1) if len(f) else np.zeros(0, bool)
    if fin.any() and not np.array_equal(np.asarray(got["aabb"], np.float32),
                                        np.concatenate([f[fin].min(0), f[fin].max(0)])):
        bad.append("aabb")
    h = hashlib.sha256()
    for a in (got["centroid"], np.float32(got["base"]), np.float32(got["threshold"]), gp, gi, got["aabb"]):
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(b"%d %d" % (int(got["count"]), int(bool(got["used_fallback"]))))
    print("case", json.dumps({"case": case, "bad": bad, "digest": h.hexdigest(), "count": int(got["count"])}), flush=True)


for c in sys.argv[2].split(","):
    run(c)
# which kernels does this route launch?  (two more small calls, profiled: the calls above ran without the events)
ops.set_profiling(True)
for case in ("n131072", "n4096"):
    raw, _ = build(case)
    ops.ground_filter(torch.from_numpy(raw).cuda())
    print("kernels", json.dumps({case: sorted({k for k, _, _ in ops.get_profile()})}), flush=True)
'''


@pytest.fixture(scope="module")
def routes(cuda):
    """{route: ({case: record}, {profiled case: kernel names}, exit status, end of stderr)}.  One child after the other; a
    child that does not end cleanly is the last one started."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    drop = ("PCH_GF_BRACKET_INVALID", "PCH_GF_NO_CAND", "PCH_MEAN_NO_PREDICT")
    out = {name: ({}, None, None, "not started: a route before it did not end cleanly") for name in ROUTES}
    for name in ("bracket", "rows"):
        env = {k: v for k, v in os.environ.items() if k not in drop}
        env.update(ROUTES[name])
        p = subprocess.run([sys.executable, "-c", CHILD, root, ",".join(CASES)], env=env, capture_output=True,
                           text=True, timeout=300)
        recs, kernels = {}, {}
        for ln in p.stdout.splitlines():
            if ln.startswith("case "):
                r = json.loads(ln[5:])
                recs[r["case"]] = r
            elif ln.startswith("kernels "):
                kernels.update(json.loads(ln[8:]))
        out[name] = (recs, kernels, p.returncode, p.stderr[-2000:])
        if p.returncode != 0:
            break
    return out


@pytest.mark.parametrize("case", CASES)
def test_ground_filter_equals_the_oracle_on_every_bracket_route(routes, case):
    digests = {}
    for name, (recs, _, rc, err) in routes.items():
        assert case in recs, f"route {name}: no result (exit {rc})\n{err}"
        assert recs[case]["bad"] == [], f"route {name} differs from oracle.ground_filter in {recs[case]['bad']}"
        digests[name] = recs[case]["digest"]
    assert len(set(digests.values())) == 1, digests


def test_the_toggles_choose_the_routes(routes):
    """Both routes gather from the summary and never sample or sweep a z column; a cloud too small for the summary's
    estimate runs the three histogram passes over the rows and gathers nothing."""
    for name, (_, kernels, rc, err) in routes.items():
        assert rc == 0 and set(kernels) == {"n131072", "n4096"}, f"route {name}: exit {rc}\n{err}"
        k = kernels["n131072"]
        assert "sel_collect" in k and "sel_bracket" not in k and "sel_sample" not in k, (name, k)
        k = kernels["n4096"]
        assert {"sel_hist0", "sel_hist1", "sel_hist2"} <= set(k), (name, k)
        assert not {"sel_collect", "sel_sample", "sel_bracket"} & set(k), (name, k)
