"""tests/gain_model.py, the reference of the two-sided what-if records
(orh_whatif_gain_rec), pinned on hand-written rows and checked on the oracle's
rows of the random cases that test_gpu_whatif_gain.py runs on the device (no
GPU here).

The random cases are the request families of whatif_lower_model on the
topologies of test_gpu_whatif_lower._random_case (28 nodes: rows of whole
quads) and on a 30-node variant (N % 4 != 0). This file also proves that those
cases are not vacuous: every class occurs, and some request has farther and
nearer nodes at once.
"""
import random

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.types import K_TESTING_AREA

from gain_model import (FIELDS, REC, SHARED, gain_classes, gain_record, node_counts, record_of, records_of,
                        zero_record)
from impact_model import INF, NO_NODE, impact_record
from test_gpu_parity import random_topology
from whatif_lower_model import changed_dbs, effective_lowers, request_families
from whatif_raise_model import Graph, effective_raises

A = K_TESTING_AREA
# (seed, nodes) of the random cases; the GPU test runs the same ones
CASES = [(1, 28), (3, 30)]
# families of request_families whose requests do nothing but lower metrics
LOWERS_ONLY = ("single", "same", "sets", "thrice")


def to_row(ref, names, nbrs):
    """run_spf_ignoring's {node: (metric, first hops)} as (dist, mask) arrays:
    node ids are positions in ``names``, mask bits positions in ``nbrs``."""
    pos = {x: i for i, x in enumerate(names)}
    bit = {x: b for b, x in enumerate(nbrs)}
    dist, nh = np.full(len(names), INF, np.uint32), np.zeros(len(names), np.uint32)
    for v, (metric, hops) in ref.items():
        dist[pos[v]] = metric
        nh[pos[v]] = sum(1 << bit[h] for h in hops)
    return dist, nh


class OracleCase:
    """One random case: the topology, 4 sources, the request families by link
    key, and the oracle's row of every request and of every source (the base
    rows), as run_spf_ignoring returns them."""

    def __init__(self, oracle, seed, n):
        self.dbs = random_topology(6100 + seed, n=n, extra=40, max_metric=12, parallel=0.25, overload=0.1,
                                   link_overload=0.08)
        self.graph = Graph(self.dbs)
        rng = random.Random(seed)
        self.srcs = rng.sample(self.graph.nodes, 4)
        self.reqs, self.marks = request_families(self.graph, rng, len(self.srcs))
        cache = {}

        def topo(drain=(), eff_r=None, eff_l=None):
            eff_r, eff_l = eff_r or {}, eff_l or {}
            key = (frozenset(drain), frozenset(eff_r.items()), frozenset(eff_l.items()))
            if key not in cache:
                cache[key] = load_topology(oracle, changed_dbs(self.dbs, eff_r, eff_l, set(drain)), [])[0][A]._impl
            return cache[key]

        self.base = {s: topo().run_spf_ignoring(s, []) for s in self.srcs}
        self.rows = []
        for k, ignore, drain, raises, lowers in self.reqs:
            ls = topo(drain, effective_raises(self.graph, raises), effective_lowers(self.graph, lowers))
            self.rows.append(ls.run_spf_ignoring(self.srcs[k], [(x[0][0], x[0][1], x[1][0]) for x in ignore]))

    def classes(self, names, nbrs_of):
        """gain_classes per request with node ids by ``names`` and the mask
        bits of source s by ``nbrs_of[s]``."""
        base = {s: to_row(self.base[s], names, nbrs_of[s]) for s in self.srcs}
        return [gain_classes(*base[self.srcs[r[0]]], *to_row(row, names, nbrs_of[self.srcs[r[0]]]),
                             names.index(self.srcs[r[0]])) for r, row in zip(self.reqs, self.rows)]

    def family(self, i):
        return next(f for f, (lo, hi) in self.marks.items() if lo <= i < hi)


_CASES = {}


def oracle_case(oracle, seed, n):
    """The case, computed once per session and never changed."""
    if (seed, n) not in _CASES:
        _CASES[seed, n] = OracleCase(oracle, seed, n)
    return _CASES[seed, n]


def case_weights(names, seed):
    """Per-node weights {name: weight} with zeros and values >= 2^31: sums pass 32 bits."""
    rng = random.Random(seed + 77)
    return {x: rng.choice((0, 1, 64, 0x80000000, 0xFFFFFFFF, rng.randrange(1 << 32))) for x in sorted(names)}


def suite_conditions(all_classes):
    """Over lists of gain_classes results: the classes that occur at all, and
    whether some request has farther and nearer nodes at once."""
    seen = {f for cs in all_classes for c in cs for f in c._fields[:6] if getattr(c, f).any()}
    both = any(c.farther.any() and c.nearer.any() for cs in all_classes for c in cs)
    return seen, both


# ---- hand rows ---------------------------------------------------------------
#        node:     0    1    2    3    4    5    6    7    8
BASE = (np.array([0, 2, 5, 4, 4, 6, INF, 7, 3], np.uint32), np.array([0, 1, 1, 3, 1, 2, 0, 3, 1], np.uint32))
REQ = (np.array([0, 2, 3, 6, 4, INF, 9, 7, 3], np.uint32), np.array([9, 1, 3, 1, 3, 0, 1, 1, 2], np.uint32))


def test_hand_rows_hit_every_class():
    """Source 0 (its own entry never counts, whatever its mask word). 1 is
    unchanged; 2 goes 5 -> 3 and gains a hop (nearer, widened); 3 goes 4 -> 6
    and loses one (farther, narrowed); 4, 7 and 8 keep their distance with
    another mask (rehomed: 4 widened, 7 narrowed, 8 neither); 5 is lost; 6 is
    unreached in the base row, so in no class although the request reaches it."""
    rec = gain_record(*BASE, *REQ, src=0)
    assert tuple(rec) == FIELDS
    assert rec == dict(lost=1, farther=1, nearer=1, rehomed=3, narrowed=2, widened=2, max_stretch=2, worst_node=3,
                       max_gain=2, best_node=2, sum_stretch=2, sum_gain=2, lost_weight=0, moved_weight=0,
                       nearer_weight=0)
    w = np.array([1000, 1, 2, 4, 8, 16, 32, 64, 128], np.uint32)
    rec = gain_record(*BASE, *REQ, src=0, weight=w)
    assert (rec["lost_weight"], rec["moved_weight"], rec["nearer_weight"]) == (16, 2 + 4 + 8 + 16 + 64 + 128, 2)
    c = gain_classes(*BASE, *REQ, src=0)
    same = gain_classes(*BASE, *BASE, src=0)
    assert record_of(same, w) == zero_record()
    lost, moved, nearer = node_counts([c, same, c])
    assert lost.tolist() == [0, 0, 0, 0, 0, 2, 0, 0, 0]
    assert moved.tolist() == [0, 0, 2, 2, 2, 2, 0, 2, 2]
    assert nearer.tolist() == [0, 0, 2, 0, 0, 0, 0, 0, 0]
    assert REC.itemsize == 80 and REC.names == FIELDS


def test_sums_past_32_bits():
    """64 nodes behind source 0, weight 2^32 - 1 each: the odd ones get nearer
    by 2^31, the even ones farther by 2^31, so the three weight sums and both
    distance sums need their 64 bits."""
    n = 65
    bd = np.full(n, 0x90000000, np.uint32)
    rd = np.where(np.arange(n) % 2 == 1, 0x10000000, 0xFFFFFFFE).astype(np.uint32)
    bd[0] = rd[0] = 0
    nh = np.ones(n, np.uint32)
    w = np.full(n, 0xFFFFFFFF, np.uint32)
    rec = gain_record(bd, nh, rd, nh, src=0, weight=w)
    assert rec["nearer"] == rec["farther"] == 32 and rec["lost"] == rec["rehomed"] == 0
    assert rec["max_gain"] == 0x80000000 and rec["best_node"] == 1
    assert rec["max_stretch"] == 0x6FFFFFFE and rec["worst_node"] == 2
    assert rec["sum_gain"] == 32 * 0x80000000 > 0xFFFFFFFF
    assert rec["sum_stretch"] == 32 * 0x6FFFFFFE > 0xFFFFFFFF
    assert rec["nearer_weight"] == 32 * 0xFFFFFFFF > 0xFFFFFFFF
    assert rec["moved_weight"] == 64 * 0xFFFFFFFF and rec["lost_weight"] == 0
    rd[1::2] = INF
    rec = gain_record(bd, nh, rd, np.where(rd == INF, 0, nh).astype(np.uint32), src=0, weight=w)
    assert rec["lost"] == 32 and rec["lost_weight"] == 32 * 0xFFFFFFFF and rec["nearer"] == 0


def test_ties_take_the_smallest_node():
    bd = np.array([0, 9, 9, 9, 9, 9, 9], np.uint32)
    rd = np.array([0, 8, 6, 12, 6, 12, 11], np.uint32)
    nh = np.ones(7, np.uint32)
    rec = gain_record(bd, nh, rd, nh, src=0)
    assert (rec["max_gain"], rec["best_node"], rec["max_stretch"], rec["worst_node"]) == (3, 2, 3, 3)
    # the source is skipped even where it would win
    rec = gain_record(bd, nh, rd, nh, src=2)
    assert (rec["max_gain"], rec["best_node"]) == (3, 4)


def test_rows_without_a_nearer_node_agree_with_the_impact_model():
    req = (np.where(REQ[0] < BASE[0], BASE[0], REQ[0]), REQ[1])
    w = np.arange(9, dtype=np.uint32) * 0x30000000 + 7
    rec, imp = gain_record(*BASE, *req, src=0, weight=w), impact_record(*BASE, *req, src=0, weight=w)
    assert rec["farther"] and rec["lost"] and rec["rehomed"] and rec["widened"]
    assert {f: rec[f] for f in SHARED} == imp
    assert (rec["nearer"], rec["max_gain"], rec["best_node"], rec["sum_gain"], rec["nearer_weight"]) == \
        (0, 0, NO_NODE, 0, 0)


# ---- the oracle's rows of the random cases -----------------------------------
@pytest.mark.parametrize("seed,n", CASES)
def test_random_cases_on_the_oracle_rows(oracle, seed, n):
    case = oracle_case(oracle, seed, n)
    names = case.graph.nodes
    assert len(names) == n < 32  # the node list doubles as every source's bit order
    classes = case.classes(names, {s: names for s in case.srcs})
    weights = case_weights(names, seed)
    w = np.array([weights[x] for x in names], np.uint32)
    n_shared = 0
    for i, (c, r) in enumerate(zip(classes, case.reqs)):
        rec = record_of(c, w)
        s = case.srcs[r[0]]
        bd, bn = to_row(case.base[s], names, names)
        rd, rn = to_row(case.rows[i], names, names)
        # the definitions once more, node by node in plain python
        nearer = [v for v in range(n) if names[v] != s and bd[v] != INF and rd[v] != INF and rd[v] < bd[v]]
        assert rec["nearer"] == len(nearer)
        assert rec["sum_gain"] == sum(int(bd[v]) - int(rd[v]) for v in nearer)
        assert rec["nearer_weight"] == sum(int(w[v]) for v in nearer)
        if nearer:
            best = max(nearer, key=lambda v: (int(bd[v]) - int(rd[v]), -v))
            assert (rec["max_gain"], rec["best_node"]) == (int(bd[best]) - int(rd[best]), best)
        else:
            imp = impact_record(bd, bn, rd, rn, names.index(s), w)
            assert {f: rec[f] for f in SHARED} == imp
            assert (rec["max_gain"], rec["best_node"], rec["sum_gain"]) == (0, NO_NODE, 0)
            n_shared += 1
        assert rec["widened"] == sum(1 for v in range(n) if names[v] != s and bd[v] != INF and rd[v] != INF and
                                     bin(rn[v]).count("1") > bin(bn[v]).count("1"))
        if case.family(i) in LOWERS_ONLY:
            assert rec["lost"] == rec["farther"] == 0, (i, r)
        assert 0 <= rec["sum_stretch"] and rec["max_stretch"] <= rec["sum_stretch"]
    assert n_shared and n_shared < len(classes)
    # each case alone has every class and mixes both directions
    seen, both = suite_conditions([classes])
    assert seen == {"lost", "farther", "nearer", "rehomed", "narrowed", "widened"} and both, (seen, both)
    recs = records_of(classes, w)
    assert recs["nearer_weight"].max() > 0xFFFFFFFF and recs["nearer"].dtype == np.uint32
    ties = sum(1 for c in classes if c.nearer.any() and (c.gain == c.gain.max()).sum() >= 2)
    assert ties, "no request ties for max_gain"


def test_random_cases_are_not_vacuous(oracle):
    """What test_gpu_whatif_gain.py relies on: over its random cases every
    class is non-zero and some request has farther and nearer nodes at once."""
    all_classes = []
    for seed, n in CASES:
        case = oracle_case(oracle, seed, n)
        all_classes.append(case.classes(case.graph.nodes, {s: case.graph.nodes for s in case.srcs}))
    seen, both = suite_conditions(all_classes)
    assert seen == {"lost", "farther", "nearer", "rehomed", "narrowed", "widened"} and both
