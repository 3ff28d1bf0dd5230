"""The what-if repair tiers and the lower pass at their capacity and tile
edges (``-m gpu``): requests with exactly cap, cap + 1 nodes or edges at every
hand-off between tiers, the two-tier plan that only ORH_REPAIR_CAPS reaches,
persistent workgroups that take several requests in a row, and
whatif_copy_kernel beyond one tile on both of its paths.

tests/whatif_sets.py has the graph family, the cases and the model that says
how many nodes and edges a request re-derives and which tier therefore ends
it; test_whatif_sets.py proves the cases' sizes on the CPU. Here every
request's info word must be the model's (tier | nodes << 3; a lowered row:
5 | (stage 1's nodes + |M|) << 3) and its row the oracle's
(run_spf_ignoring on a topology loaded with the request's changes), compared
by helpers.row_digest, so repeated requests have equal rows.

ORH_REPAIR_CAPS is read when the process's context is created, so every cap
setting runs in a fresh child process, one at a time, which writes the info
words and row digests of all its batches into an .npz for the parent to
compare (the shape of test_gpu_whatif_knobs.py). A child that fails fails its
test, and no further child is started.

  no variable set       tier 1 against tier 2 at 256 nodes / 1,024 edges
  ORH_REPAIR_CAPS=64,256    no tier 1: tier 2 drains queue 0, the slots
                        queue 1 (tier_plan's two-tier plan), also with
                        ORH_WHATIF_FULL=4 (full searches behind that plan)
  ORH_REPAIR_CAPS=300,1100  tier 1, tier 2 and the slots in one run; a request
                        that leaves tier 1 by its edges reaches tier 2 with
                        list indices in its mask row

Every case runs as a batch of ignored links (masks only, and distances
moving), one with drains and one with raises (the kDrain / kRaise
instantiations), interleaved with tier-0 requests, with share_base off and on.
No request can leave tier 1 by its edges and tier 2 by its nodes: tier 1's
node cap is never above tier 2's.
"""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.types import K_TESTING_AREA

import whatif_sets as ws
from helpers import row_digest
from test_gpu_whatif_impact import to_row
from test_gpu_whatif_lower import Oracles
from whatif_raise_model import link_key

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEARCH, LOWERED = 4, 5  # ORH_WHATIF_TIER_SEARCH, ORH_WHATIF_TIER_LOWERED
# one graph and its batches: (label, share_base, source index per request, request dicts)
Job = collections.namedtuple("Job", "name dbs srcs batches rows", defaults=(False,))


def _shares(label, idx, reqs):
    return [(f"{label} share={int(share)}", share, idx, reqs) for share in (False, True)]


def jobs(mode):
    """The graphs and batches of a child process, the same in parent and child."""
    what, _, setting = mode.partition(":")
    out = []
    if what == "repair":
        for case in ws.SETTINGS[setting]["cases"]:
            batches = []
            for kind, reqs in ws.case_batches(case):
                batches += _shares(kind, [0] * len(reqs), [r for r, _, _, _ in reqs])
            out.append(Job(case.name, case.chain.dbs(), [ws.S], batches))
    elif what == "lower":
        for case in ws.LOWER_SETTINGS[setting]["cases"]:
            reqs = [r for r, _, _, _ in ws.lower_batch(case)]
            out.append(Job(case.name, case.chain.dbs(), [ws.S], _shares("lower", [0] * len(reqs), reqs)))
    elif what == "reuse":
        reqs = [ws.REUSE_KINDS[i % 4][0] for i in range(ws.REUSE_REQUESTS)]
        out.append(Job("reuse", ws.REUSE_CHAIN.dbs(), [ws.S], [("cycle", False, [0] * len(reqs), reqs)]))
    elif what == "full":
        batches = [(kind, False, [0] * len(reqs), [r for r, _, _, _ in reqs]) for kind, reqs in ws.full_batches()]
        out.append(Job(ws.FULL_CASE.name, ws.FULL_CASE.chain.dbs(), [ws.S], batches))
    elif what == "copy":
        for n in ws.COPY_NODES:
            reqs = ws.copy_requests(n)
            out.append(Job(f"path{n}", ws.path_dbs(n), ws.copy_sources(n),
                           _shares("copy", [k for k, *_ in reqs], [r for _, r, *_ in reqs]), True))
    else:
        raise ValueError(mode)
    return out


def child_main(mode, out):
    """In the child: every batch of the mode run, info words and row digests
    (whole rows where the job asks for them) saved by job and batch."""
    from openr_amd import host_backend
    res = {}
    for job in jobs(mode):
        als, _ = load_topology(host_backend(), job.dbs, [])
        ls = als[A]._impl
        lid = {link_key(d): l for l, d in ls.link_ids()}

        def changes(reqs, what):
            return [[(lid[k], end, m) for k, end, m in r.get(what, ())] for r in reqs]
        for label, share, idx, reqs in job.batches:
            drain = [list(r.get("drain", ())) for r in reqs]
            metric, lower = changes(reqs, "metric"), changes(reqs, "lower")
            b = ls.what_if_batch(job.srcs, idx, [[lid[k] for k in r.get("ignore", ())] for r in reqs], len(reqs),
                                 share_base=share, drain=drain if any(drain) else None,
                                 metric=metric if any(metric) else None, lower=lower if any(lower) else None)
            b.run()
            b.sync()
            rows = [b.fetch(i) for i in range(len(reqs))]
            key = f"{job.name}|{label}|"
            res[key + "info"] = np.asarray(b.info(), dtype=np.uint32)
            res[key + "digest"] = np.array([row_digest(d, m) for d, m in rows], dtype=np.uint64)
            if job.rows:
                res[key + "dist"] = np.stack([d for d, _ in rows])
                res[key + "nh"] = np.stack([m for _, m in rows])
            del b
    np.savez(out, **res)


_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import test_gpu_whatif_caps as t
t.child_main(sys.argv[3], sys.argv[2])
"""
_failed = []  # the modes whose child process failed: nothing is started after one


def _child(tmp_path, mode, caps=None, **env):
    if _failed:
        pytest.fail(f"not started: the child process of {_failed[0]} failed")
    out = tmp_path / "out.npz"
    env = dict(env, ORH_REPAIR_CAPS="%d,%d" % caps) if caps else env
    base = {k: v for k, v in os.environ.items() if not k.startswith(("ORH_WHATIF_", "ORH_REPAIR_"))}
    try:
        subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out), mode], check=True, env=dict(base, **env),
                       timeout=120)
    except (subprocess.CalledProcessError, subprocess.TimeoutExpired):
        _failed.append(mode)
        raise
    return np.load(out)


class Expect:
    """A job in the parent: the model's sets and the oracle's row per distinct request."""

    def __init__(self, hip, oracle, job):
        als, _ = load_topology(hip, job.dbs, [])
        self.ls = als[A]._impl
        self.job = job
        self.desc = dict(self.ls.link_ids())
        self.lid = {link_key(d): l for l, d in self.desc.items()}
        self.oracles = Oracles(oracle, job.dbs, self.desc)
        self.graph = self.oracles.graph
        self.names = self.ls.node_names()
        self.nbrs = {s: self.ls.neighbors(s) for s in job.srcs}
        self.base = {s: ws.distances(self.graph, s) for s in job.srcs}
        self.cache = {}

    def __call__(self, k, req):
        """((|A|, E of A, |M|, E of M), (dist, mask) of the oracle's row, its digest)."""
        key = (k, repr(sorted(req.items())))
        if key not in self.cache:
            s = self.job.srcs[k]

            def changes(what):
                return [(self.lid[x], end, m) for x, end, m in req.get(what, ())]
            ref = self.oracles(req.get("drain", ()), changes("metric"), changes("lower"))._impl.run_spf_ignoring(
                s, [self.desc[self.lid[x]][:3] for x in req.get("ignore", ())])
            row = to_row(ref, self.names, self.nbrs[s])
            self.cache[key] = (ws.request_sets(self.graph, s, self.base[s], req), row, row_digest(*row))
        return self.cache[key]


def _info(sets, caps):
    n_a, e_a, n_m, _ = sets
    tier = ws.expected_tier(n_a, e_a, *caps)
    return LOWERED | (n_a + n_m) << 3 if n_m else tier | n_a << 3


def _check(hip, oracle, mode, got, caps, full=0):
    """Every batch of the mode: the info words are the model's and the rows
    the oracle's. full: the slot-bound requests of a batch are tier 3 with
    their count, or, 1 to `full` of them, tier 4. Returns the tiers seen."""
    seen = collections.Counter()
    for job in jobs(mode):
        want = Expect(hip, oracle, job)
        for label, _, idx, reqs in job.batches:
            key = f"{job.name}|{label}|"
            info, digest = got[key + "info"], got[key + "digest"]
            assert len(info) == len(digest) == len(reqs)
            shown, searched = set(), 0
            for i, req in enumerate(reqs):
                sets, row, ref = want(idx[i], req)
                model = _info(sets, caps)
                if repr(req) not in shown and len(shown) < 8:
                    shown.add(repr(req))
                    print(f"{mode} {job.name} {label} #{i}: model (nodes {sets[0]}, edges {sets[1]}, M {sets[2]}, "
                          f"its edges {sets[3]}, tier {model & 7}) device (count {int(info[i]) >> 3}, "
                          f"tier {int(info[i]) & 7})")
                where = (mode, job.name, label, i, req, sets)
                if full and (model & 7) == 3 and info[i] == SEARCH:
                    searched += 1
                else:
                    assert int(info[i]) == model, where
                assert int(digest[i]) == ref, where
                if job.rows:
                    dist, nh = got[key + "dist"][i], got[key + "nh"][i]
                    edge = slice(4093, 4099)  # round the first tile's end
                    assert np.array_equal(dist[-3:], row[0][-3:]) and np.array_equal(nh[-3:], row[1][-3:]), where
                    assert np.array_equal(dist[edge], row[0][edge]) and np.array_equal(nh[edge], row[1][edge]), where
                    assert np.array_equal(dist, row[0]) and np.array_equal(nh, row[1]), where
                seen[int(info[i]) & 7] += 1
            if full:
                assert 1 <= searched <= full, (mode, job.name, label, searched)
    return seen


@pytest.mark.parametrize("setting", ["small", "two", "three"])
def test_repair_at_the_caps(hip, oracle, tmp_path, setting):
    """cap - 1, cap and cap + 1 nodes; cap, cap + 1 and cap + 2 edges under
    the node cap; both caps at once - at tier 1's caps with no variable set
    (small), at tier 2's in the two-tier plan of ORH_REPAIR_CAPS=64,256 (two),
    and at both behind each other under 300,1100 (three), where one batch ends
    at tiers 3, 2, 1 and 0."""
    spec = ws.SETTINGS[setting]
    got = _child(tmp_path, "repair:" + setting, spec["caps"])
    seen = _check(hip, oracle, "repair:" + setting, got, spec["tier2"])
    assert set(seen) == {"small": {0, 1, 2}, "two": {0, 2, 3}, "three": {0, 1, 2, 3}}[setting]


@pytest.mark.parametrize("setting", ["two", "default"])
def test_lower_at_the_caps(hip, oracle, tmp_path, setting):
    """|M| at cap - 1, cap, cap + 1 and its edges at cap and cap + 1 of the
    lower pass's LDS state (64 / 256 by ORH_REPAIR_CAPS; 2,048 / 8,192 with no
    variable set): the LDS pass, the zero-mask marks and the slot pass that
    reads them back; a lower that moves nothing; and a request whose stage 1
    repaired the chain, which stage 2 re-derives again."""
    spec = ws.LOWER_SETTINGS[setting]
    got = _child(tmp_path, "lower:" + setting, spec["caps"])
    seen = _check(hip, oracle, "lower:" + setting, got, spec["caps"] or ws.DEFAULT_CAPS)
    assert set(seen) == {0, 2, 3, LOWERED}
    # A lowered row's word does not say which pass ended it. What pins the caps
    # (the default ones above all) is the batch's request without a lower: it
    # re-derives the same set in stage 1, whose tier 2 has the same caps, so it
    # reports tier 2 up to the caps and tier 3 past them
    alone = next(i for i, (req, *_) in enumerate(ws.lower_batch(spec["cases"][0])) if "lower" not in req)
    for case in spec["cases"]:
        for share in (0, 1):
            assert int(got[f"{case.name}|lower share={share}|info"][alone]) == case.tier | case.nodes << 3, case.name


def test_workgroups_take_several_requests(hip, oracle, tmp_path):
    """8,192 requests on one 70-node graph under 64,256, in turn one that
    fits tier 2, one that outgrows its node list, one that outgrows its edge
    list, and a tier-0 one: 6,144 queued requests for at most 8 workgroups per
    CU, then 4,096 for the 64 slots, so every workgroup clears its membership
    bitmap, through the list or whole, in front of requests of the other kinds."""
    got = _child(tmp_path, "reuse", (64, 256))
    seen = _check(hip, oracle, "reuse", got, (64, 256))
    n = ws.REUSE_REQUESTS // 4
    assert seen == {0: n, 2: n, 3: 2 * n}


def test_full_searches_in_the_two_tier_plan(hip, oracle, tmp_path):
    """ORH_REPAIR_CAPS=64,256 ORH_WHATIF_FULL=4, a batch of ignored links and
    one with drains: 1 to 4 of the requests that outgrow tier 2 are searched
    in full (the search reads queue 1, which the slot tier drains in this
    plan), the others repaired in slots; tiers 0 and 2 as without the switch."""
    got = _child(tmp_path, "full", (64, 256), ORH_WHATIF_FULL="4")
    seen = _check(hip, oracle, "full", got, (64, 256), full=4)
    assert set(seen) == {0, 2, 3, SEARCH}


def test_copy_beyond_one_tile(hip, oracle, tmp_path):
    """Paths of 4,097, 4,099 (N % 4 != 0: the scalar loop, two tiles) and 4,100
    nodes (the vector loop, a last tile of one uint4), 8 requests from two
    sources, four of them tier 0, with share_base off (every row copied) and on
    (only the queued ones): every row in full."""
    got = _child(tmp_path, "copy")
    seen = _check(hip, oracle, "copy", got, ws.DEFAULT_CAPS)
    assert seen[0] == 4 * 2 * len(ws.COPY_NODES) and set(seen) == {0, 1, 2, 3}
    # the cut at the middle of the 4,097-node path re-derives 2,048 nodes
    # (tier 2), of the others 2,049 (tier 3): the default caps are 2,048
    for n in ws.COPY_NODES:
        nodes = 2048 if n == 4097 else 2049
        k = [r[2] for r in ws.copy_requests(n)].index(nodes)
        assert int(got[f"path{n}|copy share=0|info"][k]) == (2 if n == 4097 else 3) | nodes << 3
