"""A plain reference of route selection, selection diff and RibPolicy over a
selection, as include/openr_hip.h specifies them (orh_route_select,
orh_route_diff, orh_route_policy), written from that contract and from the
reference's

  createRouteForPrefix up to the first-hop set     Decision.cpp:445-613
  selectBestRoutes / maybeFilterDrainedNodes        Decision.cpp:794-862
  getMinCostNodes / getNextHopsWithMetric           Decision.cpp:1152-1228
  selectBestPrefixMetrics                           Util.h:491-526
  RibPolicyStatement::match / applyAction,
  RibPolicy::applyPolicy                            RibPolicy.cpp:73-158, 229-247

Pure Python over numpy arrays: Python integers do the arithmetic and the
32-bit fields of the ABI are masked where they are 32-bit. Nothing here is
derived from the kernels; tests/test_route_model.py pins this model to the
oracle and to the reference's known answers, tests/test_gpu_route_kernels.py
compares the kernels with it.

Data shapes
  prefix   (prefix_flags, [adv, ...])       an empty list is a withdrawn prefix
  adv      (name, meta, path_pref, source_pref, distance)       one orh_adv
  area     dict(present, dist, nh, ovl, name_node, words, word_off): `dist`
           [N] u32 or None (me is not in the area), `nh` [N][words] u32,
           `ovl` [N], `name_node` [n_names] (NO_NODE: the name is not a node
           of this area)
"""
import numpy as np

SEL_NONE, SEL_ROUTE, SEL_HOST = 0, 1, 2
SELECT_BEST_ROUTE, SELECT_V4 = 1, 2
NO_NODE = 0xFFFFFFFF
UNREACHABLE = 0xFFFFFFFF
AREA_MASK = 0xFF
ADV_SR_MPLS, ADV_KSP2, ADV_BGP, ADV_MIN_NEXTHOP, ADV_PREPEND = 1 << 8, 1 << 9, 1 << 10, 1 << 11, 1 << 12
TAGSET_SHIFT, TAGSET_OVF = 13, 0x7FFFF
PFX_V4 = 1
MAX_ADV_DEVICE = 64  # longer lists are ORH_SEL_HOST (orh_route_select)
POL_NONE, POL_HOST, POL_MAX_STMTS = 0xFF, 0xFE, 32


def _i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def metrics_key(path_pref, source_pref, distance):
    """The tuple selectBestPrefixMetrics maximises (Util.h:503-506). Its last
    element is `distance * -1` in the reference's int32: taken here in
    wrapping 32-bit arithmetic, so INT32_MIN negates to itself (the smallest
    key, i.e. the worst distance), which is what two's-complement hardware
    gives the reference too."""
    return (_i32(path_pref), _i32(source_pref), _i32(-_i32(distance)))


def best_metrics(advs, among):
    """selectBestPrefixMetrics: the positions in `among` whose key is the
    maximum."""
    if not among:
        return []
    keys = {i: metrics_key(*advs[i][2:5]) for i in among}
    top = max(keys.values())
    return [i for i in among if keys[i] == top]


def _node(area, name, n_names):
    if name >= n_names:
        return NO_NODE
    return int(area["name_node"][name])


def select_one(pflags, advs, areas, me_name, flags, name_rank, area_rank, total_words):
    """One prefix: (status, metric, best, mask[total_words]). For NONE and
    HOST the metric is UNREACHABLE and the mask is zero; `best` is only
    meaningful for ROUTE (None otherwise)."""
    n_names = len(name_rank)
    n_areas = len(areas)
    zero = [0] * total_words
    none = (SEL_NONE, UNREACHABLE, None, zero)
    host = (SEL_HOST, UNREACHABLE, None, zero)
    if not advs:  # no entry in PrefixState (:453-456)
        return none
    if len(advs) > MAX_ADV_DEVICE:
        return host

    # entries of unreachable nodes leave (:467-480). An entry of an area the
    # solver has no LinkState of is never erased, and `me` is in its own
    # SpfResult; both are cases the host keeps.
    reach, keeps = [], False
    for i, (name, meta, _pp, _sp, _d) in enumerate(advs):
        ar = meta & AREA_MASK
        if ar >= n_areas or not areas[ar]["present"]:
            reach.append(i)
            keeps = True
            continue
        if name == me_name:
            reach.append(i)
            keeps = True
            continue
        A = areas[ar]
        if A["dist"] is None:
            continue
        v = _node(A, name, n_names)
        if v != NO_NODE and int(A["dist"][v]) != UNREACHABLE:
            reach.append(i)
    if not reach:  # :483-488
        return none
    if (pflags & PFX_V4) and not (flags & SELECT_V4):  # :491-499
        return none
    if keeps or any(advs[i][1] & ADV_BGP for i in reach):  # :501-546
        return host

    # selectBestRoutes (:804-819)
    sel = best_metrics(advs, reach) if flags & SELECT_BEST_ROUTE else list(reach)
    # bestNodeArea = *allNodeAreas.begin(): std::set<NodeAndArea> order, i.e.
    # (name string, area string), given here by the two rank tables
    best = min(sel, key=lambda i: (int(name_rank[advs[i][0]]), int(area_rank[advs[i][1] & AREA_MASK])))
    # maybeFilterDrainedNodes (:840-862): overloaded in the entry's own area;
    # bestNodeArea stays
    undrained = []
    for i in sel:
        A = areas[advs[i][1] & AREA_MASK]
        if not int(A["ovl"][_node(A, advs[i][0], n_names)]):
            undrained.append(i)
    chosen = undrained or sel

    # getPrefixForwardingTypeAndAlgorithm (Util.cpp:452-480): the minimum of
    # each over the chosen entries (IP < SR_MPLS, SP_ECMP < KSP2_ED_ECMP);
    # getMinNextHopThreshold (:824-838): set when any chosen entry sets it
    if all(advs[i][1] & ADV_SR_MPLS for i in chosen):
        return host
    if all(advs[i][1] & ADV_KSP2 for i in chosen):
        return host
    if any(advs[i][1] & ADV_MIN_NEXTHOP for i in chosen):
        return host

    # getNextHopsWithMetric (:1182-1228): per area getMinCostNodes over the
    # chosen *names* (:1159 drops the area of the entry)
    names = {advs[i][0] for i in chosen}
    per_area = []
    shortest = UNREACHABLE
    for A in areas:
        if not A["present"] or A["dist"] is None:
            per_area.append((UNREACHABLE, []))
            continue
        m, nodes = UNREACHABLE, []
        for name in names:
            v = _node(A, name, n_names)
            if v == NO_NODE:
                continue
            d = int(A["dist"][v])
            if d == UNREACHABLE:  # not in the SpfResult
                continue
            if d < m:
                m, nodes = d, []
            if d == m:
                nodes.append(v)
        per_area.append((m, nodes))
        shortest = min(shortest, m)
    if shortest == UNREACHABLE:
        return (SEL_NONE, UNREACHABLE, best, zero)
    mask = [0] * total_words
    for A, (m, nodes) in zip(areas, per_area):
        if m != shortest:
            continue
        for v in nodes:
            for w in range(A["words"]):
                mask[A["word_off"] + w] |= int(A["nh"][v][w]) & 0xFFFFFFFF
    if not any(mask):
        return (SEL_NONE, UNREACHABLE, best, zero)
    return (SEL_ROUTE, shortest, best, mask)


def select(prefixes, areas, me_name, flags, name_rank, area_rank, total_words=None):
    """orh_route_select over a whole prefix set: status[n] u8, metric[n] u32,
    best[n] (int64; -1 where the contract leaves it open, i.e. not ROUTE),
    mask[n][total_words] u32."""
    if total_words is None:
        total_words = max([A["word_off"] + A["words"] for A in areas] + [0])
    n = len(prefixes)
    status = np.zeros(n, np.uint8)
    metric = np.zeros(n, np.uint32)
    best = np.full(n, -1, np.int64)
    mask = np.zeros((n, total_words), np.uint32)
    for p, (pflags, advs) in enumerate(prefixes):
        s, m, b, k = select_one(pflags, advs, areas, me_name, flags, name_rank, area_rank, total_words)
        status[p], metric[p] = s, m
        if s == SEL_ROUTE:
            best[p] = b
        mask[p] = k
    return status, metric, best, mask


def diff(cur, prev, n, prev_n):
    """orh_route_diff: the records {p, status, metric, best, mask...} of cur
    for every p < n that is new (p >= prev_n) or whose route changed. A route
    is its status and, for ROUTE, its metric, best advertisement and mask:
    what the other fields of a NONE / HOST record hold is not part of it."""
    cs, cm, cb, ck = cur
    ps, pm, pb, pk = prev
    out = set()
    for p in range(n):
        if p < min(prev_n, n):
            same = int(cs[p]) == int(ps[p])
            if same and int(cs[p]) == SEL_ROUTE:
                same = (int(cm[p]) == int(pm[p]) and int(cb[p]) == int(pb[p])
                        and [int(x) for x in ck[p]] == [int(x) for x in pk[p]])
            if same:
                continue
        out.add((p, int(cs[p]), int(cm[p]) & 0xFFFFFFFF, int(cb[p]) & 0xFFFFFFFF) + tuple(int(x) for x in ck[p]))
    return out


def policy(sel, advs, pol, lo, hi):
    """orh_route_policy_range over prefixes [lo, hi): (out[hi - lo] u8,
    invalidated). sel = (status, metric, best, mask) of the selection, advs[p]
    the advertisement list of prefix p, pol a dict with the fields of
    orh_policy (n_stmts, stmt_tags, stmt_prefixes, tagset_stmts, pfx_id,
    pfx_stmts, keep[n_stmts][words])."""
    status, _metric, best, mask = sel
    n_stmts = pol["n_stmts"]
    assert n_stmts <= POL_MAX_STMTS
    named = {int(p): int(s) for p, s in zip(pol["pfx_id"], pol["pfx_stmts"])}
    tagsets = [int(x) for x in pol["tagset_stmts"]]
    any_tag_stmt = any((pol["stmt_tags"] >> s) & 1 for s in range(n_stmts))
    out = np.full(hi - lo, POL_NONE, np.uint8)
    invalidated = 0
    for p in range(lo, hi):
        if int(status[p]) != SEL_ROUTE:  # applyPolicy runs over routes
            continue
        ts = (advs[p][int(best[p])][1] & 0xFFFFFFFF) >> TAGSET_SHIFT
        if ts == TAGSET_OVF and any_tag_stmt:
            out[p - lo] = POL_HOST  # the tags have no id: the host matches them
            continue
        meets = tagsets[ts] if ts < len(tagsets) else 0
        names = named.get(p, 0)
        for s in range(n_stmts):  # applyPolicy (:229-247): first statement that applies
            has_t = (pol["stmt_tags"] >> s) & 1
            has_p = (pol["stmt_prefixes"] >> s) & 1
            # match (:73-105): no matcher at all never matches
            if not (has_t or has_p):
                continue
            if has_t and not (meets >> s) & 1:
                continue
            if has_p and not (names >> s) & 1:
                continue
            # applyAction (:108-158): nexthops of weight 0 are dropped; if
            # that drops all of them the route stays as it was and counts
            if any(int(mask[p][w]) & int(pol["keep"][s][w]) for w in range(len(mask[p]))):
                out[p - lo] = s
                break
            invalidated += 1
    return out, invalidated
