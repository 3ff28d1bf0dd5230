"""The set model of tests/whatif_sets.py, on the CPU: every named case of the
cap tests (test_gpu_whatif_caps.py) has exactly the set sizes and the tier it is
meant to have, so the shapes are proven before a GPU runs them; and on random
topologies the model's sets hold every node whose oracle row changes.
"""
import random

import pytest

from openr_amd.facade import load_topology
from openr_amd.types import K_TESTING_AREA

import whatif_sets as ws
from test_gpu_parity import random_topology
from test_whatif_metric_model import make_requests
from whatif_lower_model import changed_dbs, effective_lowers, request_families
from whatif_raise_model import Graph, effective_raises

A = K_TESTING_AREA


def _graph(chain):
    graph = Graph(chain.dbs())
    assert len(graph.nodes) == chain.nodes
    base = ws.distances(graph, ws.S)
    assert len(base) == chain.nodes  # every node is reached
    return graph, base


def test_expected_tier():
    for caps in ((2048, 8192), (1024, 4096), (300, 1100)):  # a tier 1 exists
        assert ws.expected_tier(0, 0, *caps) == 0
        assert ws.expected_tier(256, 1024, *caps) == 1
        assert ws.expected_tier(257, 1024, *caps) == (2 if caps[0] >= 257 else 3)
        assert ws.expected_tier(256, 1025, *caps) == 2
        assert ws.expected_tier(caps[0], caps[1], *caps) == 2
        assert ws.expected_tier(caps[0] + 1, 0, *caps) == 3
        assert ws.expected_tier(1, caps[1] + 1, *caps) == 3
    for caps in ((64, 256), (256, 1024), (100, 1024)):  # none: its state would be no smaller
        assert ws.expected_tier(0, 0, *caps) == 0
        assert ws.expected_tier(1, 1, *caps) == 2
        assert ws.expected_tier(caps[0], caps[1], *caps) == 2
        assert ws.expected_tier(caps[0] + 1, 1, *caps) == 3
        assert ws.expected_tier(1, caps[1] + 1, *caps) == 3


@pytest.mark.parametrize("setting", sorted(ws.SETTINGS))
def test_repair_cases_have_their_sizes(setting):
    """Per case and request: the model's (|A|, E) and tier are the table's, and
    the table's are the closed forms n (+1), 2 (p (n - 1) + j) (+1)."""
    spec = ws.SETTINGS[setting]
    ca, ce = spec["tier2"]
    names = [c.name for c in spec["cases"]]
    assert len(set(names)) == len(names)
    tiers = set()
    for case in spec["cases"]:
        graph, base = _graph(case.chain)
        assert (case.nodes, case.edges) == case.chain.whole()
        for cut in case.cuts:
            assert (cut.nodes, cut.edges) == case.chain.below(cut.k)
        assert base[ws.Z] == 1 and base[case.chain.c(case.chain.n)] == case.chain.n + 1
        for kind, reqs in ws.case_batches(case):
            assert any(t == 0 for _, _, _, t in reqs)
            for req, nodes, edges, tier in reqs:
                n_a, e_a, n_m, _ = ws.request_sets(graph, ws.S, base, req)
                assert (n_a, e_a, n_m) == (nodes, edges, 0), (case.name, kind, req)
                assert ws.expected_tier(n_a, e_a, ca, ce) == tier, (case.name, kind, req)
                tiers.add(tier)
    assert tiers == ({0, 2, 3} if setting == "two" else {0, 1, 2} if setting == "small" else {0, 1, 2, 3})
    # the caps themselves and one past them, by nodes and by edges
    bound = (256, 1024) if setting == "small" else (ca, ce)
    sizes = {(c.nodes, c.edges) for c in spec["cases"]}
    assert {n for n, _ in sizes} >= {bound[0] - 1, bound[0], bound[0] + 1}
    assert {e for n, e in sizes if n < bound[0]} >= {bound[1], bound[1] + 1, bound[1] + 2}
    assert bound in sizes
    assert any(c.chain.nodes % 4 for c in spec["cases"])


def test_widths_of_the_family():
    """ELL width 4 (90 % of the nodes have at most 4 records), width 8, and a
    node with more than 8 records, all among the cases."""
    def degrees(chain):
        graph = Graph(chain.dbs())
        return sorted(len(graph.out[x]) for x in graph.nodes)
    shapes = set()
    for spec in ws.SETTINGS.values():
        for case in spec["cases"]:
            deg = degrees(case.chain)
            shapes.add((8 if deg[len(deg) * 9 // 10] > 4 else 4, deg[-1] > 8))
    assert {(4, False), (8, False), (8, True)} <= shapes


@pytest.mark.parametrize("setting", sorted(ws.LOWER_SETTINGS))
def test_lower_cases_have_their_sizes(setting):
    spec = ws.LOWER_SETTINGS[setting]
    ca, ce = spec["caps"] or ws.DEFAULT_CAPS
    for case in spec["cases"]:
        graph, base = _graph(case.chain)
        assert (case.nodes, case.edges) == case.chain.whole()
        assert base[case.chain.c(1)] == 5
        assert case.tier == (2 if case.nodes <= ca and case.edges <= ce else 3)  # 2: the LDS pass holds M
        for req, stage1, n_m, e_m in ws.lower_batch(case):
            got = ws.request_sets(graph, ws.S, base, req)
            assert (got[0], got[2], got[3]) == (stage1, n_m, e_m), (case.name, req)
            if stage1:
                assert got[1] == case.edges
    sizes = {(c.nodes, c.edges) for c in spec["cases"]}
    assert {n for n, _ in sizes} >= {ca - 1, ca, ca + 1} and {e for _, e in sizes} >= {ce, ce + 1}


def test_reuse_kinds_have_their_sizes():
    graph, base = _graph(ws.REUSE_CHAIN)
    for req, nodes, edges, tier in ws.REUSE_KINDS:
        n_a, e_a, _, _ = ws.request_sets(graph, ws.S, base, req)
        assert (n_a, e_a) == (nodes, edges) and ws.expected_tier(n_a, e_a, 64, 256) == tier
    assert [t for _, _, _, t in ws.REUSE_KINDS] == [2, 3, 3, 0]
    assert ws.REUSE_KINDS[1][1] > 64 and ws.REUSE_KINDS[2][1] <= 64 < 256 < ws.REUSE_KINDS[2][2]


def test_full_batches_have_their_sizes():
    """The batches of the full-search test: 9 requests each outgrow tier 2
    under 64,256, and requests of tiers 0 and 2 stand between them."""
    graph, base = _graph(ws.FULL_CASE.chain)
    kinds = []
    for kind, reqs in ws.full_batches():
        kinds.append(kind)
        tiers = []
        for req, nodes, edges, tier in reqs:
            n_a, e_a, _, _ = ws.request_sets(graph, ws.S, base, req)
            assert (n_a, e_a) == (nodes, edges) and ws.expected_tier(n_a, e_a, 64, 256) == tier, (kind, req)
            tiers.append(tier)
        assert tiers.count(3) == 9 and {0, 2} <= set(tiers)
    assert kinds == ["ignore", "drain"]


@pytest.mark.parametrize("n", ws.COPY_NODES)
def test_copy_requests_have_their_sizes(n):
    """The path graphs of the copy test: four tier-0 requests, two of one and
    two nodes, one of all but two, and the cut at the middle, which re-derives
    exactly 2,048 nodes of the 4,097 (tier 2) and 2,049 of the others."""
    graph = Graph(ws.path_dbs(n))
    srcs = ws.copy_sources(n)
    base = {s: ws.distances(graph, s) for s in srcs}
    assert len(graph.nodes) == n and all(len(b) == n for b in base.values())
    reqs = ws.copy_requests(n)
    for k, req, nodes, edges, tier in reqs:
        n_a, e_a, _, _ = ws.request_sets(graph, srcs[k], base[srcs[k]], req)
        assert (n_a, e_a) == (nodes, edges) and ws.expected_tier(n_a, e_a, *ws.DEFAULT_CAPS) == tier, (k, req)
    sizes = sorted(nodes for _, _, nodes, _, _ in reqs)
    assert sizes == [0, 0, 0, 0, 1, 2, 2048 if n == 4097 else 2049, n - 2]
    assert sorted(t for *_, t in reqs) == [0, 0, 0, 0, 1, 1, 2 if n == 4097 else 3, 3]
    assert {k for k, *_ in reqs} == {0, 1}


def _changed(row, ref):
    return {v for v in set(row) | set(ref) if row.get(v) != ref.get(v)}


@pytest.mark.parametrize("seed", range(4))
def test_sets_hold_every_changed_node(oracle, seed):
    """Brute force on the 28-node random topologies: a node whose oracle row
    differs from the base row is in A (ignored links, drains, raises); one whose
    row differs between the graph without and with the lowers is in M."""
    dbs = random_topology(6100 + seed, n=28, extra=40, max_metric=12, parallel=0.25, overload=0.1,
                          link_overload=0.08)
    graph = Graph(dbs)
    rng = random.Random(seed)
    plain, _ = load_topology(oracle, dbs, [])
    cache = {}

    def rows(src, ignore, drain, eff_r, eff_l):
        key = (frozenset(drain), frozenset(eff_r.items()), frozenset(eff_l.items()))
        if key not in cache:
            cache[key] = load_topology(oracle, changed_dbs(dbs, eff_r, eff_l, set(drain)), [])[0][A]
        return cache[key]._impl.run_spf_ignoring(src, [(k[0][0], k[0][1], k[1][0]) for k in ignore])

    hit = 0
    for src, ignore, drain, raises in make_requests(graph, rng, 60):
        base = plain[A]._impl.run_spf_ignoring(src, [])
        dist = {v: d for v, (d, _) in base.items()}
        assert dist == ws.distances(graph, src)
        eff = effective_raises(graph, raises)
        a, e = ws.affected_set(graph, src, dist, ignore, drain, eff)
        changed = _changed(base, rows(src, ignore, drain, eff, {}))
        assert changed <= a, (src, ignore, drain, raises)
        assert e <= sum(len(graph.out[v]) for v in a)
        hit += bool(changed)
    assert hit >= 10
    srcs = rng.sample(graph.nodes, 4)
    fam, _ = request_families(graph, rng, len(srcs), mixed=10)
    hit = 0
    for k, ignore, drain, raises, lowers in rng.sample(fam, 150):
        eff_r, eff_l = effective_raises(graph, raises), effective_lowers(graph, lowers)
        m, _ = ws.lowered_set(graph, srcs[k], ignore, drain, eff_r, eff_l)
        changed = _changed(rows(srcs[k], ignore, drain, eff_r, {}), rows(srcs[k], ignore, drain, eff_r, eff_l))
        assert changed <= m, (srcs[k], ignore, drain, raises, lowers)
        hit += bool(changed)
    assert hit >= 10
