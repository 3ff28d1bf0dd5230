"""Metric lowers in what-if jobs (orh_whatif_run_lowers: costing a link back
in) against the oracle (``-m gpu``).

A request may lower the metric that one end, or both ends, of a link advertise
(Link::setMetricFromNode, LinkState.cpp:640-710), next to its ignored links,
drained nodes and raises. Stage 1 of the job is the repair without the lowers;
stage 2 (whatif_lower_kernels.hip) lets distances fall from the lowered records
and re-derives the first-hop masks of every node that got nearer or gained an
equal-cost path. The reference for every row is the oracle's runSpf on a
topology loaded with the changed metrics (and the drained nodes overloaded):
metric and first-hop set of every node, unreached nodes absent.
"""
import ctypes as C
import dataclasses
import random

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid, int_topology
from openr_amd.types import K_TESTING_AREA

from test_gpu_parity import random_topology
from test_gpu_whatif_drain import _view, orh_csr
from whatif_lower_model import changed_dbs, effective_lowers, request_families
from whatif_raise_model import Graph, effective_raises, link_key

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
NO_NODE = 0xFFFFFFFF
LOWERED = 5  # ORH_WHATIF_TIER_LOWERED


class Oracles:
    """The oracle LinkState per distinct (drain set, effective raises,
    effective lowers): the adjacency databases with the changing ends' metrics
    replaced and isOverloaded set on the drained nodes, loaded afresh."""

    def __init__(self, oracle, dbs, desc):
        self.oracle, self.dbs, self.desc, self.cache = oracle, dbs, desc, {}
        self.graph = Graph(dbs)

    def keyed(self, changes):
        return [(link_key(self.desc[l]), end, m) for l, end, m in changes]

    def __call__(self, drain=(), metric=(), lower=()):
        eff_r = effective_raises(self.graph, self.keyed(metric))
        eff_l = effective_lowers(self.graph, self.keyed(lower))
        key = (frozenset(drain), frozenset(eff_r.items()), frozenset(eff_l.items()))
        if key not in self.cache:
            als, _ = load_topology(self.oracle, changed_dbs(self.dbs, eff_r, eff_l, set(drain)), [])
            self.cache[key] = als[A]
        return self.cache[key]


class Requests:
    """Parallel per-request lists in what_if_batch's form."""

    def __init__(self):
        self.idx, self.ignore, self.drain, self.metric, self.lower = [], [], [], [], []

    def add(self, k, ignore=(), drain=(), metric=(), lower=()):
        self.idx.append(k), self.ignore.append(list(ignore)), self.drain.append(list(drain))
        self.metric.append(list(metric)), self.lower.append(list(lower))
        return len(self.idx) - 1

    def __len__(self):
        return len(self.idx)

    def batch(self, ls, srcs, chunk=None, lowers=True, **kw):
        return ls.what_if_batch(srcs, self.idx, self.ignore, chunk or max(len(self), 1),
                                drain=self.drain if any(self.drain) else None,
                                metric=self.metric if any(self.metric) else None,
                                lower=self.lower if lowers else None, **kw)

    def run(self, ls, srcs, **kw):
        b = self.batch(ls, srcs, **kw)
        b.run()
        b.sync()
        return b


def _check_rows(ls, batch, oracles, srcs, rq, which=None):
    names = ls.node_names()
    nbrs = {s: ls.neighbors(s) for s in srcs}
    for i in (range(len(rq)) if which is None else which):
        s = srcs[rq.idx[i]]
        d, m = batch.fetch(i)
        ref = oracles(rq.drain[i], rq.metric[i], rq.lower[i])._impl.run_spf_ignoring(
            s, [oracles.desc[l][:3] for l in rq.ignore[i]])
        assert _view(names, nbrs[s], d, m) == ref, (i, s, rq.lower[i], rq.metric[i], rq.drain[i], rq.ignore[i])


def _random_case(hip, oracle, seed):
    """The topology, sources and request families of the model test
    (test_whatif_lower_model.py), by link id, from each of 4 sources."""
    dbs = random_topology(6100 + seed, n=28, extra=40, max_metric=12, parallel=0.25, overload=0.1,
                          link_overload=0.08)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    desc = dict(ls.link_ids())
    oracles = Oracles(oracle, dbs, desc)
    graph = oracles.graph
    assert graph.down and graph.overloaded
    lid = {link_key(d): l for l, d in desc.items()}
    assert set(lid) == {k for k, _ in graph.metric}
    rng = random.Random(seed)
    srcs = rng.sample(graph.nodes, 4)
    fam, marks = request_families(graph, rng, len(srcs))
    rq = Requests()
    for k, ignore, drain, raises, lowers in fam:
        rq.add(k, [lid[x] for x in ignore], drain, [(lid[x], e, m) for x, e, m in raises],
               [(lid[x], e, m) for x, e, m in lowers])
    return ls, oracles, srcs, rq, marks


@pytest.mark.parametrize("seed", range(6))
def test_lower_random_graphs(hip, oracle, seed):
    """Every link lowered from each end and from both, to cur - 1, (cur + 1) //
    2 and 1, from each of 4 sources; to the current value (info 0); sets of 2-3
    lowers; lowers mixed with an ignored link, a drained node, a raise of
    another link; the same (link, end) three times; a link both lowered and
    ignored. Seed 5 also runs as a hop-count job: lowers and raises do nothing
    there, so the words and rows are those of the same requests with their
    ignored links and drained nodes alone, and 0 where a request has neither."""
    ls, oracles, srcs, rq, marks = _random_case(hip, oracle, seed)
    b = rq.run(ls, srcs)
    _check_rows(ls, b, oracles, srcs, rq)
    info = b.info()
    assert np.any((info & 7) == LOWERED) and not np.any((info & 7) == 4)
    assert np.all(info[slice(*marks["same"])] == 0)
    if seed != 5:
        return
    del b
    hop = rq.run(ls, srcs, use_link_metric=False)
    plain = ls.what_if_batch(srcs, rq.idx, rq.ignore, len(rq), use_link_metric=False, drain=rq.drain)
    plain.run()
    plain.sync()
    info = hop.info()
    assert np.array_equal(info, plain.info())
    bare = [i for i in range(len(rq)) if not rq.ignore[i] and not rq.drain[i]]
    assert len(bare) > len(rq) // 2 and np.all(info[bare] == 0)
    for i in range(len(rq)):
        (d, m), (pd, pm) = hop.fetch(i), plain.fetch(i)
        assert np.array_equal(d, pd) and np.array_equal(m, pm), (i, rq.lower[i])


def _lid(ls, a, b):
    return next(lid for lid, d in ls.link_ids() if {d[0], d[2]} == {a, b})


def _hand(hip, oracle, adj, reqs, overloaded=()):
    """Source "0" on int_topology(adj): the requests' rows (checked against
    the oracle) in run_spf_ignoring's form, and their info words. reqs: dicts
    of Requests.add's keywords with links as (a, b) name pairs."""
    dbs = [dataclasses.replace(db, isOverloaded=db.thisNodeName in overloaded) for db in int_topology(adj)]
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    rq = Requests()
    for r in reqs:
        rq.add(0, [_lid(ls, *x) for x in r.get("ignore", [])], r.get("drain", []),
               [(_lid(ls, *x), e, m) for x, e, m in r.get("metric", [])],
               [(_lid(ls, *x), e, m) for x, e, m in r.get("lower", [])])
    b = rq.run(ls, ["0"])
    _check_rows(ls, b, Oracles(oracle, dbs, dict(ls.link_ids())), ["0"], rq)
    names, nbrs = ls.node_names(), ls.neighbors("0")
    return [_view(names, nbrs, *b.fetch(i)) for i in range(len(rq))], [int(x) for x in b.info()]


def test_lower_equal_path_widens_masks(hip, oracle):
    """(a) 0-1-3 costs 3 and 0-2-3 costs 2; 3-4-5-6 hangs below. Lowering
    1 -> 3 to 1 makes the ways equal: no distance moves, the masks of 3 and of
    the three nodes below it widen, and the word counts those four."""
    adj = {0: [(1, 1), (2, 1)], 1: [(0, 1), (3, 2)], 2: [(0, 1), (3, 1)], 3: [(1, 2), (2, 1), (4, 1)],
           4: [(3, 1), (5, 1)], 5: [(4, 1), (6, 1)], 6: [(5, 1)]}
    rows, info = _hand(hip, oracle, adj, [{}, {"lower": [(("1", "3"), "1", 1)]}, {"lower": [(("1", "3"), "3", 1)]}])
    base, got, far_end = rows
    for v, d in (("3", 2), ("4", 3), ("5", 4), ("6", 5)):
        assert base[v] == (d, ["2"]) and got[v] == (d, ["1", "2"])
    assert far_end == base  # 3 -> 1 is on no path from 0
    assert info == [0, LOWERED | 4 << 3, 0]


def test_lower_into_no_transit_nodes(hip, oracle):
    """(b) 2 is overloaded, 5 is drained by its request. A lowered record into
    either brings that node nearer and nothing below it moves: 3 stays where
    it is behind the overloaded 2, and 3 and 6, which the drain sent round over
    4 (stage 1), stay there behind the drained 5."""
    adj = {0: [(1, 1), (4, 1)], 1: [(0, 1), (2, 5)], 2: [(1, 5), (3, 1)], 3: [(2, 1), (4, 9), (6, 1)],
           4: [(0, 1), (3, 9), (5, 5)], 5: [(4, 5), (6, 1)], 6: [(5, 1), (3, 1)]}
    rows, info = _hand(hip, oracle, adj, [{}, {"lower": [(("1", "2"), "1", 1)]},
                                          {"drain": ["5"], "lower": [(("4", "5"), "4", 1)]}], overloaded=("2",))
    base, into_ovl, into_drained = rows
    assert base["2"] == (6, ["1"]) and base["3"] == (8, ["4"]) and base["5"] == (6, ["4"]) and base["6"] == (7, ["4"])
    assert into_ovl["2"] == (2, ["1"]) and {v: x for v, x in into_ovl.items() if v != "2"} == \
        {v: x for v, x in base.items() if v != "2"}
    assert into_drained["5"] == (2, ["4"]) and into_drained["3"] == (10, ["4"]) and into_drained["6"] == (11, ["4"])
    assert info == [0, LOWERED | 1 << 3, LOWERED | 3 << 3]  # 6 and 3 by the drain, 5 by the lower


def test_lower_out_of_the_source_and_behind_an_ignored_link(hip, oracle):
    """(c) 2 is reached over 1 at 2; lowering 0 -> 2 from 5 to 1 makes it a
    neighbour route: its mask becomes its own bit. (e) 3 and 4 hang off 1 by
    the link 1-3 alone; with that link ignored, a lowered 3 -> 4 starts at an
    unreached tail and nothing happens."""
    adj = {0: [(1, 1), (2, 5)], 1: [(0, 1), (2, 1), (3, 1)], 2: [(0, 5), (1, 1)], 3: [(1, 1), (4, 7)], 4: [(3, 7)]}
    rows, info = _hand(hip, oracle, adj, [
        {}, {"lower": [(("0", "2"), "0", 1)]},
        {"ignore": [("1", "3")]},
        {"ignore": [("1", "3")], "lower": [(("3", "4"), "3", 1)]},
    ])
    base, direct, cut, cut_lower = rows
    assert base["2"] == (2, ["1"]) and direct["2"] == (1, ["2"]) and direct["1"] == (1, ["1"])
    assert set(cut) == {"0", "1", "2"} and cut_lower == cut
    assert info[:2] == [0, LOWERED | 1 << 3]
    assert info[2] == info[3] and info[2] & 7 == 1  # stage 1's word stands


def test_lower_pulls_back_part_of_a_raised_subtree(hip, oracle):
    """(d) The chain 0-1-2-3-4 at unit metrics, and 0-5-3 at 4 + 4. Raising
    0 -> 1 to 6 pushes 1..4 out; lowering 0 -> 5 and 5 -> 3 to 1 pulls them
    back from the far end: 5, 3 and 4 end below their base distance, 2 and 1
    between the base row and stage 1's."""
    adj = {0: [(1, 1), (5, 4)], 1: [(0, 1), (2, 1)], 2: [(1, 1), (3, 1)], 3: [(2, 1), (4, 1), (5, 4)],
           4: [(3, 1)], 5: [(0, 4), (3, 4)]}
    up = [(("0", "1"), "0", 6)]
    rows, info = _hand(hip, oracle, adj, [{}, {"metric": up},
                                          {"metric": up, "lower": [(("0", "5"), "0", 1), (("3", "5"), "5", 1)]}])
    base, r1, got = rows
    dist = lambda row: {v: row[v][0] for v in "12345"}
    assert dist(base) == {"1": 1, "2": 2, "3": 3, "4": 4, "5": 4}
    assert dist(r1) == {"1": 6, "2": 7, "3": 8, "4": 9, "5": 4}
    assert dist(got) == {"1": 4, "2": 3, "3": 2, "4": 3, "5": 1}
    assert all(got[v][1] == ["5"] for v in "12345")
    assert info[2] & 7 == LOWERED and info[2] >> 3 == (info[1] >> 3) + 5


def test_lower_tiers(hip, oracle):
    """60x60 grid with every metric 4, source 0 (corner). Lowering what 0
    advertises towards 1 to 1 brings every node outside column 0 nearer by 3
    (3,540 nodes, past the LDS caps: global state), each then with the single
    first hop 1; 70 copies pass the 64 slots. 40 requests lower a link next to
    the far corner (small sets, in LDS), one lowers a link to its current
    value."""
    dbs = [dataclasses.replace(db, adjacencies=[dataclasses.replace(a, metric=4) for a in db.adjacencies])
           for db in bench_grid(60, 0)[0]]
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    desc = dict(ls.link_ids())
    by_ends = {frozenset((d[0], d[2])): lid for lid, d in desc.items()}

    def right(x, value=1):
        return (by_ends[frozenset((str(x), str(x + 1)))], str(x), value)

    far = [r * 60 + c for r in range(52, 60) for c in range(54, 59)]
    assert len(far) == 40
    lows = [right(0)] * 35 + [right(x) for x in far] + [right(7, 4)] + [right(0)] * 35
    rq = Requests()
    for low in lows:
        rq.add(0, lower=[low])
    b = rq.run(ls, ["0"])
    info = b.info()
    tier, affected = info & 7, info >> 3
    big = [i for i, low in enumerate(lows) if low == right(0)]
    assert len(big) == 70
    assert np.all(tier[big] == LOWERED) and np.all(affected[big] >= 3540)
    assert np.all(tier[35:75] == LOWERED) and np.all(affected[35:75] < 256)
    assert info[75] == 0
    first = {}
    for i, low in enumerate(lows):
        first.setdefault(low, i)
    _check_rows(ls, b, Oracles(oracle, dbs, desc), ["0"], rq, which=sorted(first.values()))
    d0, m0 = b.fetch(big[0])
    names, nbrs = ls.node_names(), ls.neighbors("0")
    bit = 1 << nbrs.index("1")
    base_d, _ = b.fetch(75)
    for v, name in enumerate(names):
        if int(name) % 60:
            assert d0[v] == base_d[v] - 3 and m0[v] == bit, name
    for i in big[1:]:
        d, m = b.fetch(i)
        assert np.array_equal(d, d0) and np.array_equal(m, m0), i


def test_lower_pipeline(hip, oracle):
    """The random-graph requests in chunks of 64 (lower lists straddle chunk
    boundaries), with share_base, and through the multi-device split on one
    device: tier words and row digests per request equal the single-chunk
    run's, whose rows test_lower_random_graphs holds to the oracle."""
    ls, oracles, srcs, rq, marks = _random_case(hip, oracle, 2)
    one = rq.batch(ls, srcs)
    one.set_digests()
    one.run()
    one.sync()
    info, dig = one.info(), one.digests()
    assert np.any((info & 7) == LOWERED) and np.any(info == 0)
    del one
    for kw in ({"chunk": 64}, {"chunk": 64, "share_base": True}, {"share_base": True}):
        b = rq.batch(ls, srcs, **kw)
        b.set_digests()
        b.run()
        b.sync()
        assert np.array_equal(b.info(), info), kw
        assert np.array_equal(b.digests(), dig), kw
        del b
    sh = rq.run(ls, srcs, share_base=True)  # a lowered request owns its row, whatever its word says
    low0 = [i for i in range(len(rq)) if info[i] == 0 and oracles(lower=rq.lower[i]) is not oracles()]
    assert low0
    _check_rows(ls, sh, oracles, srcs, rq, which=low0[:50])
    del sh
    rls = hip.module.ReplicatedLinkState(A, [0, 0])
    for db in oracles.dbs:
        rls.update_adjacency_database(db.to_wire())
    assert dict(rls.replica(1).link_ids()) == dict(ls.link_ids())
    md = rls.what_if_batch(srcs, rq.idx, rq.ignore, 64, drain=rq.drain, metric=rq.metric, lower=rq.lower)
    assert md.blocks == 2
    md.set_digests()
    md.run()
    md.sync()
    assert np.array_equal(md.info(), info)
    assert np.array_equal(md.digests(), dig)


def test_lower_bad_arguments(hip):
    dbs = [dataclasses.replace(db, adjacencies=[dataclasses.replace(a, metric=4) for a in db.adjacencies])
           for db in bench_grid(4, 0)[0]]
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    lid = _lid(ls, "0", "1")

    def fails(match, exc=RuntimeError, impact=False, **kw):
        b = ls.what_if_batch(["0"], [0], [[]], 1, **kw)
        if impact:
            b.set_impact(True)
        with pytest.raises(exc, match=match):
            b.run()

    with pytest.raises(ValueError, match="unknown node"):
        ls.what_if_batch(["0"], [0], [[]], 1, lower=[[(lid, "no-such-node", 2)]])
    with pytest.raises(ValueError, match="one list of metric lowers per request"):
        ls.what_if_batch(["0"], [0, 0], [[], []], 2, lower=[[(lid, None, 2)]])
    fails(r"\(-1\).*above the current", lower=[[(lid, "0", 5)]])            # an increase
    fails(r"\(-1\).*from_node", lower=[[(lid, "5", 2)]])                    # no end of the link
    fails(r"\(-3\).*zero-metric", lower=[[(lid, "0", 0)]])
    fails(r"\(-1\).*both raised and lowered", lower=[[(lid, "0", 2)]], metric=[[(lid, None, 9)]])
    fails(r"\(-1\).*below the current", metric=[[(lid, "0", 2)]])           # a decrease is no raise
    fails("impact", exc=ValueError, impact=True, lower=[[(lid, "0", 2)]])
    ok = ls.what_if_batch(["0"], [0], [[]], 1, lower=[[(lid, "0", 2)]], metric=[[(lid, "1", 9)]])
    ok.run()
    ok.sync()
    d, _ = ok.fetch(0)
    assert d[ls.node_names().index("1")] == 2 and int(ok.info()[0]) & 7 == LOWERED


vp = C.c_void_p


def _p(a):
    return a.ctypes.data_as(vp)


def test_lower_c_abi(hip):
    """The raw library on a 5-node ring 0-1-2-3-4-0 with metrics 3 (link l
    joins l and l + 1), a down chord 1-3 (link 5) and a free link slot (6):
    every validation case with its code, none of which queues anything or
    harms the job (the next, valid, run is right); then a run without lowers
    into the same buffers, which waits for the lower pass by itself and equals
    orh_whatif_run_metrics run alone."""
    from openr_amd import HIP_LIB_PATH
    lib = C.CDLL(HIP_LIB_PATH)
    N, DOWN = 5, 0x80000000
    for name, args in {
        "orh_create": [C.c_int, C.c_uint32, C.POINTER(vp)], "orh_destroy": [vp],
        "orh_graph_create": [vp, C.POINTER(vp)], "orh_graph_destroy": [vp],
        "orh_graph_load": [vp, C.POINTER(orh_csr)],
        "orh_device_alloc": [vp, C.c_size_t, C.POINTER(vp)], "orh_device_free": [vp, vp],
        "orh_memcpy_d2h": [vp, vp, vp, C.c_size_t],
        "orh_whatif_create": [vp, vp, C.c_uint32, C.c_int32, C.POINTER(vp)],
        "orh_whatif_run_metrics": [vp, C.c_uint32] + [vp] * 10,
        "orh_whatif_run_lowers": [vp, C.c_uint32] + [vp] * 12,
        "orh_row_digest": [vp, vp, vp, C.c_uint32, C.c_uint32, C.c_uint32, vp],
        "orh_whatif_flush": [vp], "orh_whatif_destroy": [vp],
    }.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    lib.orh_last_error.argtypes, lib.orh_last_error.restype = [vp], C.c_char_p
    links = [(l, l, (l + 1) % N, 0) for l in range(N)] + [(5, 1, 3, DOWN)]
    ents = [sorted([(b if a == v else a, l | fl) for l, a, b, fl in links if v in (a, b)]) for v in range(N)]
    row_ptr = np.cumsum([0] + [len(r) for r in ents]).astype(np.uint32)
    col = np.array([c for row in ents for c, _ in row], np.uint32)
    meta = np.array([m for row in ents for _, m in row], np.uint32)
    w = np.full(len(col), 3, np.uint32)
    ovl = np.zeros(N, np.uint8)
    csr = orh_csr(N, len(col), 7, _p(row_ptr), _p(col), _p(w), _p(w), _p(meta), _p(ovl), None)
    ctx, g, job = vp(), vp(), vp()
    assert lib.orh_create(0, 0, C.byref(ctx)) == 0
    try:
        assert lib.orh_graph_create(ctx, C.byref(g)) == 0
        assert lib.orh_graph_load(g, C.byref(csr)) == 0, lib.orh_last_error(ctx)
        src = np.array([0], np.uint32)
        assert lib.orh_whatif_create(g, _p(src), 1, 1, C.byref(job)) == 0, lib.orh_last_error(ctx)
        n_max = 8
        bufs = []
        for _ in range(7):
            d = vp()
            assert lib.orh_device_alloc(ctx, n_max * N * 8, C.byref(d)) == 0
            bufs.append(d)
        d_dist, d_nh, d_info, d_dist2, d_nh2, d_dig, d_dig2 = bufs

        def get(d, count, dtype=np.uint32):
            a = np.zeros(count, dtype)
            assert lib.orh_memcpy_d2h(ctx, _p(a), d, a.nbytes) == 0
            return a

        def csr_of(lists):
            ptr = np.cumsum([0] + [len(x) for x in lists]).astype(np.uint32)
            return ptr, np.array([v for x in lists for r in x for v in r] + [0, 0, 0], np.uint32)

        def run(lowers, raises=None, ign=None, flush=True):
            """One request per entry of `lowers` (lists of (link, from, metric))."""
            n = len(lowers)
            idx = np.zeros(n, np.uint32)
            ign = ign or [[] for _ in lowers]
            ip = np.cumsum([0] + [len(x) for x in ign]).astype(np.uint32)
            il = np.array([l for x in ign for l in x] + [0], np.uint32)
            lp, ls_ = csr_of(lowers)
            mp, ms = csr_of(raises) if raises else (None, None)
            rc = lib.orh_whatif_run_lowers(job, n, _p(idx), _p(ip), _p(il), None, None,
                                           _p(mp) if raises else None, _p(ms) if raises else None, _p(lp), _p(ls_),
                                           d_dist, d_nh, d_info)
            if rc == 0 and flush:
                assert lib.orh_whatif_flush(job) == 0
            return rc

        def rows(n):
            return (get(d_dist, n * N).reshape(n, N).tolist(), get(d_nh, n * N).reshape(n, N).tolist(),
                    [int(x) for x in get(d_info, n)])

        base = ([0, 3, 6, 6, 3], [0, 1, 1, 2, 2])  # neighbours of 0: 1 (bit 0), 4 (bit 1)
        assert run([[(0, 0, 4)]]) == -1  # an increase: ORH_E_INVALID
        assert b"above the current" in lib.orh_last_error(ctx)
        assert run([[(1, NO_NODE, 2)], [(0, 3, 2)]]) == -1  # from_node is no end of the link
        assert b"from_node" in lib.orh_last_error(ctx)
        assert run([[(5, 0, 2)]]) == -1  # a down link's from_node is still checked
        assert run([[(0, 0, 0)]]) == -3  # ORH_E_UNSUPPORTED
        assert b"zero-metric" in lib.orh_last_error(ctx)
        assert run([[(0, 0, 2)]], raises=[[(0, NO_NODE, 9)]]) == -1  # raised and lowered
        assert b"both raised and lowered" in lib.orh_last_error(ctx)
        mp, ms = csr_of([[(0, 0, 2)]])  # a decrease among the raises stays what it was
        one = np.zeros(2, np.uint32)
        assert lib.orh_whatif_run_metrics(job, 1, _p(one), _p(one), _p(one), None, None, _p(mp), _p(ms),
                                          d_dist, d_nh, d_info) == -1
        assert b"below the current" in lib.orh_last_error(ctx)
        # the valid cases, in one run: 0 -> 1 lowered to 1, to 2 three times over, from both ends; to the
        # current value; link id >= n_links and a free slot; the down chord (metric 0 never looked at);
        # from the far end; lowered and ignored; 4 -> 0's far end raised next to the lower of 0 -> 1
        assert run([[(0, 0, 1)], [(0, 0, 2), (0, 0, 1), (0, 0, 3)], [(0, NO_NODE, 1)], [(0, NO_NODE, 3)],
                    [(7, 0, 1), (99, NO_NODE, 0), (6, 0, 1)], [(5, 1, 0), (5, NO_NODE, 1)], [(0, 1, 1)],
                    [(0, 0, 1)]], ign=[[]] * 7 + [[0]]) == 0, lib.orh_last_error(ctx)
        dist, nh, info = rows(8)
        lowered = ([0, 1, 4, 6, 3], [0, 1, 1, 2, 2])
        for r in (0, 1, 2):
            assert (dist[r], nh[r], info[r]) == (*lowered, LOWERED | 2 << 3), r
        for r in (3, 4, 5, 6):
            assert (dist[r], nh[r], info[r]) == (*base, 0), r
        assert (dist[7], nh[7]) == ([0, 12, 9, 6, 3], [0, 2, 2, 2, 2]) and info[7] & 7 == 1
        assert run([[(0, 0, 1)]], raises=[[(4, 0, 5)]]) == 0, lib.orh_last_error(ctx)
        dist, nh, info = rows(1)
        assert (dist[0], nh[0]) == ([0, 1, 4, 7, 5], [0, 1, 1, 1, 2]) and info[0] & 7 == LOWERED
        # a run with lowers, unflushed, then one without into the same buffers
        n = 3
        raises = [[(4, 0, 5)], [], [(0, 0, 7)]]
        assert run([[(0, 0, 1)], [(1, 1, 1)], [(4, 0, 1)]], flush=False) == 0
        mp, ms = csr_of(raises)
        idx, ip = np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32)
        assert lib.orh_whatif_run_lowers(job, n, _p(idx), _p(ip), _p(ip), None, None, _p(mp), _p(ms), None, None,
                                         d_dist, d_nh, d_info) == 0, lib.orh_last_error(ctx)
        assert lib.orh_whatif_run_metrics(job, n, _p(idx), _p(ip), _p(ip), None, None, _p(mp), _p(ms),
                                          d_dist2, d_nh2, None) == 0
        assert lib.orh_whatif_flush(job) == 0
        assert lib.orh_row_digest(ctx, d_dist, d_nh, 1, N, n, d_dig) == 0
        assert lib.orh_row_digest(ctx, d_dist2, d_nh2, 1, N, n, d_dig2) == 0
        dig = get(d_dig, n, np.uint64)
        assert np.array_equal(dig, get(d_dig2, n, np.uint64)) and len(set(dig.tolist())) == 3
        assert get(d_dist, n * N).reshape(n, N).tolist() == [[0, 3, 6, 8, 5], [0, 3, 6, 6, 3], [0, 7, 9, 6, 3]]
        assert [int(x) & 7 for x in get(d_info, n)] == [1, 0, 1]
    finally:
        if job:
            lib.orh_whatif_destroy(job)
        if g:
            lib.orh_graph_destroy(g)
        lib.orh_destroy(ctx)
