"""The repair rule for metric raises (tests/whatif_raise_model.py) against the
oracle: a request's row, derived from the plain row by the rule, equals
run_spf_ignoring on the topology whose adjacency metrics were replaced.

Runs on the CPU; the GPU kernels are held to the same oracle rows in
test_gpu_whatif_metric.py.
"""
import random

import pytest

from openr_amd.facade import load_topology
from openr_amd.types import K_TESTING_AREA

from test_gpu_parity import random_topology
from whatif_raise_model import Graph, effective_raises, raised_dbs, repair, spf, view

A = K_TESTING_AREA


def make_requests(graph, rng, count):
    """(source, ignored keys, drained nodes, raises): 1-3 raises each, from one
    end or both, by +1, x3, to 10^6 or to the current value, on up and down
    links; a third of the requests also ignore a link (now and then one they
    raise), a third drain a node."""
    keys = sorted({k for k, _ in graph.metric})
    reqs = []
    for n in range(count):
        src = rng.choice(graph.nodes)
        raises = []
        for _ in range(rng.choice((1, 1, 2, 3))):
            key = rng.choice(keys)
            end = rng.choice(graph.ends(key) + [None])
            cur = max(graph.metric[(key, t)] for t in graph.ends(key))
            raises.append((key, end, rng.choice((cur + 1, cur * 3, 10 ** 6, cur if end is None else graph.metric[(key, end)]))))
        if n % 7 == 0:
            raises.append((raises[0][0], raises[0][1], raises[0][2] + rng.randrange(5)))  # the same (link, end) twice
        ignore = []
        if n % 3 == 0:
            ignore = [raises[0][0] if n % 4 == 0 else rng.choice(keys)]
        drain = [rng.choice(graph.nodes)] if n % 3 == 1 else []
        reqs.append((src, ignore, drain, raises))
    return reqs


# seeds whose requests re-derive something in at least a quarter of the cases
@pytest.mark.parametrize("seed", range(7000, 7008))
def test_rule_matches_the_oracle(oracle, seed):
    uniform = seed % 2 == 1
    dbs = random_topology(seed, n=24, extra=34, max_metric=1 if uniform else 12, parallel=0.25,
                          overload=0.1, link_overload=0.08)
    graph = Graph(dbs)
    assert graph.down and graph.overloaded
    rng = random.Random(seed)
    base = {}
    plain, _ = load_topology(oracle, dbs, [])
    nonempty = 0
    reqs = make_requests(graph, rng, 60)
    for src, ignore, drain, raises in reqs:
        if src not in base:
            base[src] = spf(graph, src)
            assert view(base[src]) == plain[A]._impl.run_spf_ignoring(src, [])
        eff = effective_raises(graph, raises)
        got, affected = repair(graph, src, base[src], ignore, drain, eff)
        als, _ = load_topology(oracle, raised_dbs(dbs, eff, drain), [])
        descs = [(k[0][0], k[0][1], k[1][0]) for k in ignore]
        assert view(got) == als[A]._impl.run_spf_ignoring(src, descs), (src, ignore, drain, raises)
        nonempty += bool(affected)
    assert 4 * nonempty >= len(reqs), f"vacuous: {nonempty} of {len(reqs)} requests re-derive anything"


def test_equalising_raise_grows_the_first_hop_set():
    """0-1-3 costs 2, 0-2-3 costs 3: raising 1->3 by one makes them equal."""
    from openr_amd.topology import int_topology
    dbs = int_topology({0: [(1, 1), (2, 1)], 1: [(0, 1), (3, 1)], 2: [(0, 1), (3, 2)], 3: [(1, 1), (2, 2)]})
    graph = Graph(dbs)
    base = spf(graph, "0")
    assert view(base)["3"] == (2, ["1"])
    key = next(k for k, t in graph.metric if {k[0][0], k[1][0]} == {"1", "3"})
    row, affected = repair(graph, "0", base, eff=effective_raises(graph, [(key, "1", 2)]))
    assert affected == {"3"} and view(row)["3"] == (3, ["1", "2"])
    # raised from the far end only: the record 1 -> 3 keeps its weight
    row, affected = repair(graph, "0", base, eff=effective_raises(graph, [(key, "3", 9)]))
    assert not affected and row == base
    with pytest.raises(ValueError):
        effective_raises(graph, [(key, None, 0)])
