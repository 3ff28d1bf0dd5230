"""tests/route_model.py (the plain reference the route kernels are compared
with in test_gpu_route_kernels.py) pinned to the oracle and to the
reference's known answers; no GPU.

  seeded 2- and 3-area topologies (overloaded nodes, `me` absent from one
  area, names present in several areas, anycast prefixes whose advertisers
  span areas), enable_best_route_selection x enable_v4: per prefix, the
  oracle's route against the model's selection over the oracle's own SPF rows
  selectBestPrefixMetrics known answers                UtilTest.cpp:873-955
  RibPolicy known answers (as in tests/test_rib_policy.py)
                                                       RibPolicyTest.cpp:75-396

What the oracle comparison can state: ROUTE => the oracle has that route
(first-hop neighbours per area, metric, best entry), NONE => it has none.
HOST says "the host decides", and the host may decide either way (a
self-advertised prefix without prepend label has no route, Decision.cpp:571;
a BGP entry without metric vector neither, :538), so a HOST prefix asserts
nothing about the oracle's route; which prefixes must be HOST is asserted
from how they were generated.
"""
import random

import numpy as np
import pytest

import route_model as rm
from openr_amd.facade import load_topology
from openr_amd.types import (IpPrefix, PrefixEntry, PrefixForwardingAlgorithm, PrefixForwardingType,
                             PrefixMetrics, PrefixType)
from test_gpu_parity import random_topology

ME = "n0"
N = 20


def _topology(seed, n_areas):
    """Adjacency databases of n_areas areas over the same node names (so a
    name is a node of several areas); every area lacks a few nodes, the last
    of three lacks `me`."""
    rng = random.Random(seed)
    dbs, areas = [], [f"A{k + 1}" for k in range(n_areas)]
    for k, area in enumerate(areas):
        absent = {f"n{i}" for i in rng.sample(range(1, N), 3)}
        if n_areas == 3 and k == 2:
            absent.add(ME)
        for db in random_topology(seed * 10 + k, n=N, extra=18, overload=0.2):
            if db.thisNodeName in absent:
                continue
            db.area = area
            db.nodeLabel += 1000 * k  # labels are unique over the areas
            for a in db.adjacencies:
                a.adjLabel += 100000 * k
            dbs.append(db)
    return areas, dbs


def _entry(prefix, node, rng, **kw):
    m = PrefixMetrics(1, rng.randint(-1, 1), rng.randint(-1, 1), rng.randint(0, 2))
    typ = kw.pop("type", PrefixType.LOOPBACK)
    mv = (1, ((1, 2, 0, False, (7,)),)) if typ == PrefixType.BGP else None
    # data names the advertiser: the route's bestPrefixEntry tells who was best
    return PrefixEntry(prefix, typ, node.encode(), kw.pop("ft", PrefixForwardingType.IP),
                       kw.pop("fa", PrefixForwardingAlgorithm.SP_ECMP), mv, kw.pop("min_nexthop", None),
                       None, m, ())


# generated classes whose single or every entry carries the property, so the
# prefix must come out HOST whenever an entry is reachable
KINDS = ("plain", "plain", "plain", "plain", "anycast", "anycast", "v4", "bgp", "sr_mpls", "ksp2",
         "min_nexthop", "self")


def _prefixes(seed, areas):
    rng = random.Random(1000 + seed)
    out = []  # (IpPrefix, kind, [(node, area, entry)])
    for i in range(72):
        kind = KINDS[i % len(KINDS)]
        prefix = IpPrefix.of(f"10.{seed}.{i}.0/24" if kind == "v4" else f"fd00:{seed:x}:{i:x}::/64")
        n_adv = {"plain": rng.randint(1, 2), "anycast": rng.randint(3, 5)}.get(kind, rng.randint(1, 3))
        pairs = set()
        while len(pairs) < n_adv:
            pairs.add((f"n{rng.randrange(1, N)}", rng.choice(areas)))
        if kind == "self":
            pairs.add((ME, areas[0]))
        kw = {"bgp": {"type": PrefixType.BGP}, "sr_mpls": {"ft": PrefixForwardingType.SR_MPLS},
              "ksp2": {"fa": PrefixForwardingAlgorithm.KSP2_ED_ECMP, "ft": PrefixForwardingType.SR_MPLS},
              "min_nexthop": {"min_nexthop": 1}}.get(kind, {})
        advs = [(node, area, _entry(prefix, node, rng, **dict(kw))) for node, area in sorted(pairs)]
        rng.shuffle(advs)
        out.append((prefix, kind, advs))
    return out


def _model_inputs(als, areas, prefixes):
    """The model's arrays from the oracle's own state: names and areas get
    ids in string order (so the rank tables are the identity), dist / nh rows
    are me's SpfResult, bit k of an area's mask is the k-th neighbour name of
    `me` in that area in sorted order."""
    names = sorted({f"n{i}" for i in range(N)})
    name_id = {s: i for i, s in enumerate(names)}
    m_areas, nbrs = [], []
    for area in areas:
        ls = als[area]
        has = [ls.has_node(s) for s in names]
        node_of = {s: k for k, s in enumerate(s for s, h in zip(names, has) if h)}
        name_node = np.array([node_of.get(s, rm.NO_NODE) for s in names], np.uint32)
        ovl = np.zeros(len(node_of), np.uint8)
        for s, k in node_of.items():
            ovl[k] = ls.is_node_overloaded(s)
        if not ls.has_node(ME):
            m_areas.append(dict(present=1, dist=None, nh=None, ovl=ovl, name_node=name_node, words=1,
                                word_off=len(m_areas)))
            nbrs.append([])
            continue
        spf = ls.get_spf_result(ME)
        nb = sorted({h for r in spf.values() for h in r.nextHops})
        assert len(nb) <= 32
        dist = np.full(len(node_of), rm.UNREACHABLE, np.uint32)
        nh = np.zeros((len(node_of), 1), np.uint32)
        for s, r in spf.items():
            dist[node_of[s]] = r.metric
            nh[node_of[s], 0] = sum(1 << nb.index(h) for h in r.nextHops)
        m_areas.append(dict(present=1, dist=dist, nh=nh, ovl=ovl, name_node=name_node, words=1,
                            word_off=len(m_areas)))
        nbrs.append(nb)
    area_id = {a: i for i, a in enumerate(sorted(areas))}
    assert [area_id[a] for a in areas] == list(range(len(areas)))
    m_prefixes = []
    for prefix, _kind, advs in prefixes:
        recs = []
        for node, area, e in advs:
            meta = area_id[area]
            meta |= rm.ADV_SR_MPLS if e.forwardingType == PrefixForwardingType.SR_MPLS else 0
            meta |= rm.ADV_KSP2 if e.forwardingAlgorithm == PrefixForwardingAlgorithm.KSP2_ED_ECMP else 0
            meta |= rm.ADV_BGP if e.type == PrefixType.BGP else 0
            meta |= rm.ADV_MIN_NEXTHOP if e.minNexthop is not None else 0
            recs.append((name_id[node], meta, e.metrics.path_preference, e.metrics.source_preference,
                         e.metrics.distance))
        m_prefixes.append((rm.PFX_V4 if prefix.is_v4() else 0, recs))
    ranks = np.arange(len(names), dtype=np.uint32), np.arange(len(areas), dtype=np.uint32)
    return m_prefixes, m_areas, name_id[ME], ranks, nbrs


def _reaches(adv, m_areas, me_id):
    """An advertiser other than `me` that is in me's SpfResult of its area."""
    A = m_areas[adv[1] & rm.AREA_MASK]
    if adv[0] == me_id or A["dist"] is None:
        return False
    v = int(A["name_node"][adv[0]])
    return v != rm.NO_NODE and int(A["dist"][v]) != rm.UNREACHABLE


@pytest.mark.parametrize("seed,n_areas", [(1, 2), (2, 2), (3, 3), (4, 3)])
def test_model_agrees_with_oracle(oracle, seed, n_areas):
    areas, dbs = _topology(seed, n_areas)
    prefixes = _prefixes(seed, areas)
    # the oracle is not given the KSP2 prefixes: its getKthPaths needs every
    # advertiser in every area; the model must still class them HOST
    als, ps = load_topology(oracle, dbs, [adv for _, kind, advs in prefixes if kind != "ksp2" for adv in advs])
    m_prefixes, m_areas, me_id, (name_rank, area_rank), nbrs = _model_inputs(als, areas, prefixes)
    if n_areas == 3:
        assert m_areas[2]["dist"] is None
    assert any(int(A["ovl"].sum()) for A in m_areas)
    seen = {rm.SEL_NONE: 0, rm.SEL_ROUTE: 0, rm.SEL_HOST: 0}
    for best_route in (False, True):
        for v4 in (False, True):
            flags = (rm.SELECT_BEST_ROUTE if best_route else 0) | (rm.SELECT_V4 if v4 else 0)
            status, metric, best, mask = rm.select(m_prefixes, m_areas, me_id, flags, name_rank, area_rank)
            db = oracle.spf_solver(ME, v4, enable_best_route_selection=best_route).build_route_db(ME, als, ps)
            assert db is not None
            for p, (prefix, kind, advs) in enumerate(prefixes):
                where = (seed, best_route, v4, str(prefix), kind)
                route = db.unicastRoutes.get(prefix)
                seen[int(status[p])] += 1
                reachable = any(_reaches(a, m_areas, me_id) for a in m_prefixes[p][1])
                if kind in ("bgp", "sr_mpls", "ksp2", "min_nexthop") and reachable and (v4 or not prefix.is_v4()):
                    assert status[p] == rm.SEL_HOST, where
                if kind == "self" and (v4 or not prefix.is_v4()):
                    assert status[p] == rm.SEL_HOST, where
                if status[p] == rm.SEL_HOST:
                    assert kind in ("bgp", "sr_mpls", "ksp2", "min_nexthop", "self"), where
                    continue
                if status[p] == rm.SEL_NONE:
                    assert route is None, where
                    assert not mask[p].any() and metric[p] == rm.UNREACHABLE
                    continue
                assert route is not None, where
                got = [sorted({h.neighborNodeName for h in route.nextHops if h.area == a}) for a in areas]
                want = [[nb[k] for k in range(len(nb)) if int(mask[p][A["word_off"]]) >> k & 1]
                        for A, nb in zip(m_areas, nbrs)]
                assert got == want, where
                assert {h.metric for h in route.nextHops} == {int(metric[p])}, where
                node, area, entry = advs[int(best[p])]
                assert route.bestArea == area and route.bestPrefixEntry.data == node.encode(), where
                assert route.bestPrefixEntry.metrics == entry.metrics, where
    # every outcome occurred and routes are the bulk
    assert seen[rm.SEL_ROUTE] > seen[rm.SEL_HOST] > 0 and seen[rm.SEL_NONE] > 0, seen


def test_cross_area_cases_occur(oracle):
    """The seeded topologies above reach the cases the comparison is for: a
    route whose metric comes from an area other than its advertisement's, and
    a selected set that the drained filter shrinks."""
    other_area = drained = 0
    for seed, n_areas in [(1, 2), (2, 2), (3, 3), (4, 3)]:
        areas, dbs = _topology(seed, n_areas)
        prefixes = _prefixes(seed, areas)
        als, _ = load_topology(oracle, dbs, [])
        m_prefixes, m_areas, me_id, (nr, ar), _ = _model_inputs(als, areas, prefixes)
        status, _, _, mask = rm.select(m_prefixes, m_areas, me_id, 0, nr, ar)
        for p, (pflags, advs) in enumerate(m_prefixes):
            if status[p] != rm.SEL_ROUTE:
                continue
            adv_areas = {a[1] & rm.AREA_MASK for a in advs}
            other_area += any(mask[p][A["word_off"]] and b not in adv_areas for b, A in enumerate(m_areas))
            flags = [int(m_areas[a[1] & 0xFF]["ovl"][v]) for a in advs
                     if (v := int(m_areas[a[1] & 0xFF]["name_node"][a[0]])) != rm.NO_NODE]
            drained += 0 < sum(flags) < len(flags)
    assert other_area > 0 and drained > 0, (other_area, drained)


# ---- selectBestPrefixMetrics known answers (UtilTest.cpp:873-955) -----------

def _best(metrics):
    advs = [(i, 0, pp, sp, d) for i, (pp, sp, d) in enumerate(metrics)]
    return rm.best_metrics(advs, list(range(len(advs))))


def test_select_best_prefix_metrics_known_answers():
    assert _best([]) == []                                            # :871-874
    assert _best([(0, 0, 0)]) == [0]                                  # :879-885
    assert _best([(100, 0, 0), (200, 0, 0), (300, 0, 0)]) == [2]      # :891-899
    assert _best([(100, 10, 0), (100, 200, 0), (100, 30, 0)]) == [1]  # :905-913
    assert _best([(100, 10, 1), (100, 10, 2), (100, 10, 3)]) == [0]   # :918-926
    assert _best([(100, 10, 1), (100, 10, 2), (100, 10, 1), (100, 10, 1), (100, 10, 2)]) == [0, 2, 3]  # :931-943
    # :950-959 all three tie; the best node area is the smallest (node, area)
    advs = [(1, 1, 100, 10, 1), (1, 0, 100, 10, 1), (2, 0, 100, 10, 1)]
    one = dict(present=1, dist=np.array([0, 5, 5], np.uint32), nh=np.array([[0], [1], [2]], np.uint32),
               ovl=np.zeros(3, np.uint8), name_node=np.array([0, 1, 2], np.uint32), words=1, word_off=0)
    two = dict(one, word_off=1)
    s, m, b, k = rm.select_one(0, advs, [one, two], 0, rm.SELECT_BEST_ROUTE, [0, 1, 2], [0, 1], 2)
    assert (s, m, b, k) == (rm.SEL_ROUTE, 5, 1, [3, 3])


def test_distance_negates_in_32_bits():
    """-distance wraps: INT32_MIN is the worst distance, INT32_MAX the next."""
    lo, hi = -(1 << 31), (1 << 31) - 1
    assert rm.metrics_key(0, 0, lo) == (0, 0, lo)
    assert _best([(0, 0, lo), (0, 0, hi)]) == [1]
    assert _best([(0, 0, hi), (0, 0, 0), (0, 0, lo)]) == [1]


# ---- RibPolicy known answers (RibPolicyTest.cpp, as tests/test_rib_policy.py) -

def _compile(stmts, routes):
    """Statements (prefixes | None, tags | None, default, {area: w}, {nbr: w})
    and routes (prefix, tags, [(area, nbr)]) in the model's form: one mask bit
    per distinct nexthop, keep[s] = the bits whose weight is > 0."""
    hops = sorted({h for _, _, hs in routes for h in hs}, key=str)
    pids = {r[0]: p for p, r in enumerate(routes)}
    tagsets = sorted({tuple(sorted(r[1])) for r in routes})
    keep, stmt_tags, stmt_pfx, named = [], 0, 0, {}
    for s, (pfx, tags, default, by_area, by_nbr) in enumerate(stmts):
        bits = 0
        for k, (area, nbr) in enumerate(hops):
            w = default
            if area is not None:
                w = by_area.get(area, w)
            if nbr is not None:
                w = by_nbr.get(nbr, w)
            bits |= (w > 0) << k
        keep.append([bits])
        stmt_tags |= bool(tags) << s
        stmt_pfx |= bool(pfx) << s
        for x in pfx or ():
            if x in pids:
                named[pids[x]] = named.get(pids[x], 0) | 1 << s
    pol = dict(n_stmts=len(stmts), stmt_tags=stmt_tags, stmt_prefixes=stmt_pfx,
               tagset_stmts=[sum(bool(set(ts) & set(st[1] or ())) << s for s, st in enumerate(stmts))
                             for ts in tagsets],
               pfx_id=sorted(named), pfx_stmts=[named[p] for p in sorted(named)], keep=keep)
    n = len(routes)
    sel = (np.full(n, rm.SEL_ROUTE, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.int64),
           np.array([[sum(1 << hops.index(h) for h in hs)] for _, _, hs in routes], np.uint32))
    advs = [[(0, tagsets.index(tuple(sorted(tags))) << rm.TAGSET_SHIFT, 0, 0, 0)] for _, tags, _ in routes]
    return sel, advs, pol


def _apply(stmts, routes):
    sel, advs, pol = _compile(stmts, routes)
    out, inv = rm.policy(sel, advs, pol, 0, len(routes))
    return [int(x) for x in out], inv


def test_rib_policy_statement_apply_action():
    # RibPolicyTest.cpp:75-117: fd00::/64 is not named; fc00::/64 keeps the
    # default-weight and the area2 nexthops
    st = [(["fc00::/64"], None, 1, {"area1": 0, "area2": 2}, {})]
    hops = [(None, None), ("area1", None), ("area2", None)]
    assert _apply(st, [("fd00::/64", [], hops), ("fc00::/64", [], hops)]) == ([rm.POL_NONE, 0], 0)


def test_rib_policy_statement_match():
    # RibPolicyTest.cpp:119-196
    hop = [("a", None)]
    routes = [("10.0.0.0/8", ["COMMODITY:EGRESS"], hop), ("11.0.0.0/8", ["COMMODITY:EGRESS"], hop),
              ("10.0.0.0/8", ["COMMODITY:INGRESS:pod1"], hop), ("11.0.0.0/8", ["COMMODITY:INGRESS:pod1"], hop)]
    # _compile numbers routes by position; the same prefix twice needs its own ids
    def run(pfx, tags):
        res = []
        for r in routes:
            res.append(_apply([(pfx, tags, 1, {"test-area": 2}, {})], [r])[0][0] == 0)
        return res
    assert run(["10.0.0.0/8"], None) == [True, False, True, False]
    assert run(None, ["COMMODITY:EGRESS"]) == [True, True, False, False]
    assert run(["10.0.0.0/8"], ["COMMODITY:EGRESS"]) == [True, False, False, False]
    assert run([], []) == [False, False, False, False]


def test_rib_policy_first_statement_wins():
    # RibPolicyTest.cpp:257-320
    st = [(["fc01::/64"], None, 1, {"area1": 99}, {}), (["fc00::/64", "fc02::/64"], None, 1, {"area2": 99}, {})]
    hops = [("area1", None), ("area2", None)]
    assert _apply(st, [("fc01::/64", [], hops), ("fc02::/64", [], hops), ("fc03::/64", [], hops)]) == \
        ([0, 1, rm.POL_NONE], 0)


def test_rib_policy_apply_policy_invalidated():
    # RibPolicyTest.cpp:322-396: e2's only nexthop has weight 0 under s2: the
    # route is kept unchanged and counted
    st = [(["fc01::/64"], None, 1, {"area1": 99}, {"nbr3": 98}),
          (["fc00::/64", "fc02::/64"], None, 1, {"area2": 0}, {})]
    nh1, nh2, nh3 = ("area1", "nbr1"), ("area2", "nbr2"), ("area1", "nbr3")
    assert _apply(st, [("fc01::/64", [], [nh1, nh2, nh3]), ("fc02::/64", [], [nh2])]) == ([0, rm.POL_NONE], 1)


def test_policy_tagset_overflow_and_range():
    sel = (np.array([1, 1, 0, 1], np.uint8), np.zeros(4, np.uint32), np.zeros(4, np.int64),
           np.array([[1], [2], [0], [1]], np.uint32))
    advs = [[(0, rm.TAGSET_OVF << rm.TAGSET_SHIFT, 0, 0, 0)], [(0, 1 << rm.TAGSET_SHIFT, 0, 0, 0)], [],
            [(0, 9 << rm.TAGSET_SHIFT, 0, 0, 0)]]
    pol = dict(n_stmts=2, stmt_tags=1, stmt_prefixes=2, tagset_stmts=[0, 1], pfx_id=[0, 1, 3, 7],
               pfx_stmts=[2, 2, 2, 2], keep=[[1], [3]])
    out, inv = rm.policy(sel, advs, pol, 0, 4)
    assert [int(x) for x in out] == [rm.POL_HOST, 1, rm.POL_NONE, 1] and inv == 1
    pol = dict(pol, stmt_tags=0)  # no tag statement: the overflow id is decided here
    out, inv = rm.policy(sel, advs, pol, 0, 2)
    assert [int(x) for x in out] == [1, 1] and inv == 0


def test_diff_ignores_stale_fields_of_non_routes():
    cur = (np.array([0, 1, 2, 1], np.uint8), np.array([7, 5, 0, 5], np.uint32), np.array([0, 1, 0, 1]),
           np.array([[0], [3], [0], [3]], np.uint32))
    prev = (np.array([0, 1, 2, 1], np.uint8), np.array([9, 5, 1, 5], np.uint32), np.array([1, 1, 2, 0]),
            np.array([[4], [3], [5], [3]], np.uint32))
    assert rm.diff(cur, prev, 4, 4) == {(3, 1, 5, 1, 3)}
    assert rm.diff(cur, prev, 4, 3) == {(3, 1, 5, 1, 3)}
    assert rm.diff(cur, prev, 4, 0) == {(0, 0, 7, 0, 0), (1, 1, 5, 1, 3), (2, 2, 0, 0, 0), (3, 1, 5, 1, 3)}


def test_gpu_fuzz_generator_is_mostly_routes():
    """The generator of tests/test_gpu_route_kernels.py does not hide behind
    HOST / NONE: under every flags value at least half of each fuzz case's
    prefixes are ROUTE, and HOST and NONE both occur."""
    from test_gpu_route_kernels import ALL_FLAGS, fuzz_case
    for n_areas in (1, 3):
        for seed in (0, 1, 2):
            for n_prefix in (255, 257):
                c = fuzz_case(seed, n_prefix, n_areas)
                for flags in ALL_FLAGS:
                    s = rm.select(c["prefixes"], c["areas"], c["me"], flags, c["name_rank"], c["area_rank"],
                                  c["total_words"])[0]
                    counts = np.bincount(s, minlength=3)
                    assert 2 * counts[rm.SEL_ROUTE] >= n_prefix, (seed, n_prefix, n_areas, flags, counts)
                    assert counts[rm.SEL_HOST] * 25 >= n_prefix and counts[rm.SEL_NONE] > 0, counts
