"""The sets a what-if request re-derives, their sizes, and a graph family that
sets both sizes at will: what the cap tests (test_whatif_sets.py on the CPU,
test_gpu_whatif_caps.py on the GPU) share.

The repair kernels (whatif_kernels.hip) keep a request's affected set A and the
predecessor edges inside it in a state of fixed capacity, and hand a request
that outgrows it to the next tier; the lower pass (whatif_lower_kernels.hip)
does the same with its mask set M. Which tier ends a request is decided by two
numbers alone, stated here from the definitions in the kernel files' headers:

  A   the heads of the request's cut records (both records of an ignored link,
      every out-record of a drained node, every raised record) that are tight
      in the base row under the record's own weight with a tail that is the
      source or not overloaded; closed under tight out-records of nodes that
      are neither overloaded nor drained in this request.
  M   the nodes that are nearer in the graph with the lowered metrics than in
      the one without, and the heads of lowered records that are tight there
      (tail reached; the source, or neither overloaded nor drained); closed
      under records tight in the new distances and weights out of such tails.
  E   of a set X: the pairs (v in X, live record of v towards p) with p in X,
      the link not ignored, p neither overloaded nor drained. All such
      records count, not the tight ones alone.

Distances come from a Dijkstra of this module's own. Requests are dicts with
the keys ignore (link keys), drain (node names), metric and lower ((link key,
end or None, value) triples), any of them absent.

The family (chain): source S, feeders a and b, a chain c1..cn and a bypass z.
S-a, S-b, a-c1, b-c1, S-z cost 1; ci-c(i+1) are p parallel links of metric 1,
one more on the first j segments (the last j with tail=True); z-cn costs
n + 10, so z is on no shortest path and every node stays reachable whatever a
request cuts. An optional leaf, overloaded, hangs on a chain node: it is below
that node and offers no way on, so it adds one node and exactly one edge. All
of these re-derive the whole chain, |A| = n (+1), E = 2 (p (n - 1) + j) (+1):

  mask     ignore {a-c1}: distances stand, first hops shrink from {a, b} to {b}
  move     ignore {a-c1, b-c1}: every chain distance moves onto the bypass
  drain    drain a
  raise    raise a -> c1

cut(k) cuts the chain between ck and c(k+1) (all parallel links ignored, ck
drained, or all records ck -> c(k+1) raised): A = c(k+1)..cn. The lower
variant has no feeders: S-c1 is two parallel links of metric 5, the only way
in; lowering the first to 1 from S pulls the whole chain nearer, |M| = n with
the same E, and ignoring the second next to it has stage 1 repair the chain
first.
"""
import collections
import dataclasses
import heapq

from openr_amd.topology import int_topology

from whatif_lower_model import effective_lowers
from whatif_raise_model import effective_raises, link_key

INF = float("inf")
S, FA, FB, Z = "0", "1", "2", "3"
BIG = 10 ** 6


def distances(graph, src, ignore=(), drain=(), weight=None):
    """{node: distance} from src: ignored links skipped, no way on through an
    overloaded or drained node other than src, a record weighs what `weight`
    ({(key, tail): metric}) says, else its own metric."""
    ignore, drain, weight = set(ignore), set(drain) - {src}, weight or {}
    dist, heap = {src: 0}, [(0, src)]
    while heap:
        d, x = heapq.heappop(heap)
        if d > dist[x] or (x != src and (x in graph.overloaded or x in drain)):
            continue
        for r in graph.out[x]:
            if r.key in ignore:
                continue
            c = d + weight.get((r.key, x), r.w)
            if c < dist.get(r.head, INF):
                dist[r.head] = c
                heapq.heappush(heap, (c, r.head))
    return dist


def edges_inside(graph, nodes, ignore, drain):
    """E of the module docstring for the set `nodes`."""
    return sum(1 for v in nodes for r in graph.out[v]
               if r.head in nodes and r.key not in ignore and r.head not in graph.overloaded and r.head not in drain)


def _closure(graph, seeds, expands, tight):
    out, level = set(seeds), list(seeds)
    while level:
        nxt = []
        for v in level:
            if not expands(v):
                continue
            for r in graph.out[v]:
                if r.head not in out and tight(r):
                    out.add(r.head)
                    nxt.append(r.head)
        level = nxt
    return out


def affected_set(graph, src, base_dist, ignore=(), drain=(), raises=()):
    """(A, E) of a request on the base row's distances {node: distance}.
    ignore: link keys; drain: node names; raises: the (key, tail) pairs of the
    raised records (effective_raises' keys)."""
    ignore, drain, raises = set(ignore), set(drain) - {src}, set(raises)

    def tight(r):
        return r.tail in base_dist and base_dist[r.tail] + r.w == base_dist.get(r.head, INF)

    cuts = [r for x in graph.nodes for r in graph.out[x] if r.key in ignore or x in drain or (r.key, x) in raises]
    seeds = {r.head for r in cuts if tight(r) and (r.tail == src or r.tail not in graph.overloaded)}
    a = _closure(graph, seeds, lambda v: v not in graph.overloaded and v not in drain, tight)
    assert src not in a
    return a, edges_inside(graph, a, ignore, drain)


def lowered_set(graph, src, ignore=(), drain=(), raises=None, lowers=None):
    """(M, E) of stage 2 of a request. raises / lowers: {(key, tail): metric}
    (effective_raises, effective_lowers)."""
    ignore, drain = set(ignore), set(drain) - {src}
    w1 = dict(raises or {})
    w2 = {**w1, **(lowers or {})}
    d1 = distances(graph, src, ignore, drain, w1)
    d2 = distances(graph, src, ignore, drain, w2)

    def transit(x):
        return x == src or (x not in graph.overloaded and x not in drain)

    def tight(r):
        return r.key not in ignore and r.tail in d2 and d2[r.tail] + w2.get((r.key, r.tail), r.w) == d2.get(r.head, INF)

    nearer = {v for v in d2 if d2[v] < d1.get(v, INF)}
    lowered = [r for x in graph.nodes for r in graph.out[x] if (r.key, x) in (lowers or {})]
    m = _closure(graph, nearer | {r.head for r in lowered if transit(r.tail) and tight(r)}, transit, tight)
    assert src not in m
    return m, edges_inside(graph, m, ignore, drain)


def expected_tier(n_a, e, cap_a, cap_e):
    """The tier that ends a request of n_a affected nodes and e edges inside
    under ORH_REPAIR_CAPS = cap_a, cap_e (tier_plan, whatif_kernels.hip)."""
    if n_a == 0:
        return 0
    if (cap_a > 256 or cap_e > 1024) and n_a <= 256 and e <= 1024:
        return 1
    if n_a <= cap_a and e <= cap_e:
        return 2
    return 3


def request_sets(graph, src, base_dist, req):
    """(|A|, E of A, |M|, E of M) of a request dict."""
    ignore, drain = req.get("ignore", ()), req.get("drain", ())
    eff_r = effective_raises(graph, req.get("metric", ()))
    eff_l = effective_lowers(graph, req.get("lower", ()))
    a, ea = affected_set(graph, src, base_dist, ignore, drain, eff_r)
    m, em = lowered_set(graph, src, ignore, drain, eff_r, eff_l) if eff_l else (set(), 0)
    return len(a), ea, len(m), em


# ---- the family -------------------------------------------------------------

@dataclasses.dataclass(frozen=True)
class Chain:
    n: int               # chain nodes
    p: int = 1           # parallel links per segment
    j: int = 0           # segments with one link more: the first j, or the last j (tail)
    leaf: bool = False   # an overloaded leaf on the chain's middle node
    lower: bool = False  # the lower variant
    tail: bool = False

    def c(self, i):
        """Name of chain node ci, 1 <= i <= n."""
        assert 1 <= i <= self.n
        return str(3 + i)

    @property
    def leaf_name(self):
        return str(4 + self.n)

    @property
    def leaf_at(self):
        return (self.n + 1) // 2

    def width(self, i):
        """Parallel links of segment ci - c(i+1), 1 <= i < n."""
        more = i > self.n - 1 - self.j if self.tail else i <= self.j
        return self.p + (1 if more else 0)

    @property
    def nodes(self):
        return self.n + (2 if self.lower else 4) + (1 if self.leaf else 0)

    def dbs(self):
        assert self.j <= self.n - 1
        adj = collections.defaultdict(list)

        def link(x, y, w=1, count=1):
            for _ in range(count):
                adj[int(x)].append((int(y), w))
                adj[int(y)].append((int(x), w))

        if self.lower:
            link(S, self.c(1), 5, 2)
        else:
            for f in (FA, FB):
                link(S, f)
                link(f, self.c(1))
        for i in range(1, self.n):
            link(self.c(i), self.c(i + 1), 1, self.width(i))
        link(S, Z)
        link(Z, self.c(self.n), self.n + 10)
        if self.leaf:
            link(self.c(self.leaf_at), self.leaf_name)
        return [dataclasses.replace(db, isOverloaded=self.leaf and db.thisNodeName == self.leaf_name)
                for db in int_topology(dict(adj))]

    def whole(self):
        """(nodes, edges) of the set of a request that re-derives the whole chain."""
        extra = 1 if self.leaf else 0
        return self.n + extra, 2 * (self.p * (self.n - 1) + self.j) + extra

    def below(self, k):
        """(nodes, edges) of the set of cut(k): c(k+1)..cn."""
        extra = 1 if self.leaf and self.leaf_at > k else 0
        return self.n - k + extra, 2 * sum(self.width(i) for i in range(k + 1, self.n)) + extra

    # requests, by kind: "ignore", "drain" or "raise"
    def whole_request(self, kind, move=False):
        up = link(FA, self.c(1))
        if kind == "ignore":
            return {"ignore": [up, link(FB, self.c(1))] if move else [up]}
        return {"drain": [FA]} if kind == "drain" else {"metric": [(up, FA, 3)]}

    def idle_request(self, kind):
        """Tier 0: z - cn is on no shortest path."""
        far = link(Z, self.c(self.n))
        if kind == "ignore":
            return {"ignore": [far]}
        return {"drain": [Z]} if kind == "drain" else {"metric": [(far, Z, BIG)]}

    def cut_request(self, kind, k):
        x, y = self.c(k), self.c(k + 1)
        links = [link(x, y, q) for q in range(self.width(k))]
        if kind == "ignore":
            return {"ignore": links}
        return {"drain": [x]} if kind == "drain" else {"metric": [(l, x, BIG) for l in links]}

    def lower_request(self, repaired=False):
        """Lower the first S - c1 link to 1 from S; repaired: the second one
        ignored as well, so that stage 1 re-derives the chain first."""
        req = {"lower": [(link(S, self.c(1)), S, 1)]}
        if repaired:
            req["ignore"] = [link(S, self.c(1), 1)]
        return req

    def idle_lower(self):
        """An effective lower that moves nothing: z -> cn by one."""
        return {"lower": [(link(Z, self.c(self.n)), Z, self.n + 9)]}


def link(x, y, k=0):
    """Key of the k-th parallel link between the nodes named x and y (int_topology's ifNames)."""
    return link_key((x, f"{x}/{y}/{k}", y, f"{y}/{x}/{k}"))


# ---- the cases ----------------------------------------------------------------
# Per cap setting: its ORH_REPAIR_CAPS (None: the variable unset; the caps are
# then the MI355X's defaults), the caps of the tier under test, and the chains
# with the (nodes, edges, tier) their whole-chain requests are meant to show.
# `cuts`: chain positions cut on top, with the same for A = c(k+1)..cn.

# With no variable set, repair_caps and lower_caps take 2,048 / 8,192 where
# that state fits the LDS, as it does in the MI355X's 160 KB for these graphs
# (else 1,024 / 4,096). The tests that rely on it pin it: a request of 2,048
# nodes must report tier 2 and one of 2,049 tier 3.
DEFAULT_CAPS = (2048, 8192)

Case = collections.namedtuple("Case", "name chain nodes edges tier cuts", defaults=((),))
Cut = collections.namedtuple("Cut", "k nodes edges tier")

SETTINGS = {
    # tier 1 against tier 2 at 256 / 1,024; ELL width 4 (p = 1, 2), 8 (p = 3), more than 8 records (p = 5)
    "small": dict(caps=None, tier2=DEFAULT_CAPS, cases=[
        Case("a-1", Chain(255), 255, 508, 1),
        Case("a", Chain(256), 256, 510, 1),
        Case("a+1", Chain(257), 257, 512, 2, (Cut(1, 256, 510, 1), Cut(2, 255, 508, 1))),
        Case("e", Chain(250, 2, 14), 250, 1024, 1),
        Case("e+1", Chain(250, 2, 14, leaf=True), 251, 1025, 2),
        Case("e+2", Chain(250, 2, 15), 250, 1026, 2),
        Case("a,e", Chain(256, 2, 2), 256, 1024, 1),
        Case("e,k8", Chain(171, 3, 2), 171, 1024, 1),
        Case("e+2,k8", Chain(171, 3, 3), 171, 1026, 2),
    ]),
    # the two-tier plan: tier 2 drains queue 0, the slots queue 1
    "two": dict(caps=(64, 256), tier2=(64, 256), cases=[
        Case("a-1", Chain(63), 63, 124, 2),
        Case("a", Chain(64), 64, 126, 2),
        Case("a+1", Chain(65), 65, 128, 3, (Cut(1, 64, 126, 2), Cut(2, 63, 124, 2))),
        Case("e", Chain(60, 2, 10), 60, 256, 2),
        Case("e+1", Chain(60, 2, 10, leaf=True), 61, 257, 3),
        Case("e+2", Chain(60, 2, 11), 60, 258, 3),
        Case("a,e", Chain(64, 2, 2), 64, 256, 2),
        Case("e,k8", Chain(43, 3, 2), 43, 256, 2),
        Case("e+2,k8", Chain(43, 3, 3), 43, 258, 3),
        Case("e,cont", Chain(26, 5, 3), 26, 256, 2),
        Case("e+1,cont", Chain(26, 5, 3, leaf=True), 27, 257, 3),
    ]),
    # three tiers: 256 / 1,024, then 300 / 1,100, then the slots
    "three": dict(caps=(300, 1100), tier2=(300, 1100), cases=[
        Case("a-1", Chain(299), 299, 596, 2),
        Case("a", Chain(300), 300, 598, 2),
        # one batch ends at tiers 3, 2, 2, 1 and 0: every hand-off in one run
        Case("a+1", Chain(301), 301, 600, 3, (Cut(1, 300, 598, 2), Cut(44, 257, 512, 2), Cut(45, 256, 510, 1))),
        Case("e", Chain(250, 2, 52), 250, 1100, 2),  # these three leave tier 1 by edges
        Case("e+1", Chain(250, 2, 52, leaf=True), 251, 1101, 3),
        Case("e+2", Chain(250, 2, 53), 250, 1102, 3),
        Case("a,e", Chain(300, 1, 251), 300, 1100, 2),
        Case("nodes then edges", Chain(280, 2), 280, 1116, 3),  # leaves tier 1 by nodes, tier 2 by edges
        Case("e,cont", Chain(110, 5, 5), 110, 1100, 2),
        Case("e+2,cont", Chain(110, 5, 6), 110, 1102, 3),
    ]),
}

# The lower pass: |M| and its edges at the LDS caps of the pass (lower_caps:
# ORH_REPAIR_CAPS first, else DEFAULT_CAPS). The info word of a lowered row
# does not tell the LDS pass from the slot pass; the rows and counts must be
# right on both sides of the caps. `tier`: 2 where the caps hold the set, else
# 3; the caps are tier 2's as well, so it is the tier that lower_batch's
# stage-1-alone request, which re-derives the same set, must report.
LOWER_SETTINGS = {
    "two": dict(caps=(64, 256), cases=[
        Case("m-1", Chain(63, lower=True), 63, 124, 2),
        Case("m", Chain(64, lower=True), 64, 126, 2),
        Case("m+1", Chain(65, lower=True), 65, 128, 3),
        Case("e", Chain(60, 2, 10, lower=True), 60, 256, 2),
        Case("e+1", Chain(60, 2, 10, leaf=True, lower=True), 61, 257, 3),
    ]),
    "default": dict(caps=None, cases=[
        Case("m-1", Chain(2047, lower=True), 2047, 4092, 2),
        Case("m", Chain(2048, lower=True), 2048, 4094, 2),
        Case("m+1", Chain(2049, lower=True), 2049, 4096, 3),
        Case("e", Chain(2040, 2, 18, lower=True), 2040, 8192, 2),
        Case("e+1", Chain(2040, 2, 18, leaf=True, lower=True), 2041, 8193, 3),
    ]),
}

# Workgroup reuse under 64,256: one chain, four kinds of request in turn
REUSE_CHAIN = Chain(66, 2, 5, tail=True)
REUSE_KINDS = [  # (request, nodes, edges, tier)
    (REUSE_CHAIN.cut_request("ignore", 10), 56, 230, 2),  # fits
    (REUSE_CHAIN.whole_request("ignore"), 66, 270, 3),     # outgrows the node list
    (REUSE_CHAIN.cut_request("ignore", 2), 64, 262, 3),    # fits by nodes, outgrows the edge list
    (REUSE_CHAIN.idle_request("ignore"), 0, 0, 0),
]
REUSE_REQUESTS = 8192


def case_batches(case):
    """The batches of a repair case: (kind, [(request, nodes, edges, tier)]).
    Runs with drains and with raises launch instantiations of their own; every
    batch is interleaved with tier-0 requests."""
    ch = case.chain
    whole = (case.nodes, case.edges, case.tier)
    out = []
    for kind in ("ignore", "drain", "raise"):
        idle = (ch.idle_request(kind), 0, 0, 0)
        reqs = [(ch.whole_request(kind), *whole), idle]
        if kind == "ignore":
            reqs += [(ch.whole_request(kind, move=True), *whole), idle]
        else:
            reqs += [(ch.whole_request("ignore"), *whole)]  # an empty drain / raise list next to full ones
        for cut in case.cuts:
            reqs += [(ch.cut_request(kind, cut.k), cut.nodes, cut.edges, cut.tier), idle]
        reqs += [(ch.whole_request(kind), *whole)]  # a repeated request: an equal row
        out.append((kind, reqs))
    return out


def lower_batch(case):
    """The batch of a lower case: (request, stage 1's nodes, |M|, edges of M)."""
    ch = case.chain
    return [
        (ch.lower_request(), 0, case.nodes, case.edges),
        (ch.idle_lower(), 0, 0, 0),
        (ch.lower_request(repaired=True), case.nodes, case.nodes, case.edges),
        ({"ignore": [link(S, ch.c(1), 1)]}, case.nodes, 0, 0),  # stage 1 alone: no lower
        (ch.lower_request(), 0, case.nodes, case.edges),
    ]


# Full searches behind the two-tier plan (64,256 with ORH_WHATIF_FULL): the
# batches of ignored links and of drains of the 65-node chain, three times
# over, so that 9 requests of each outgrow tier 2
FULL_CASE = next(c for c in SETTINGS["two"]["cases"] if c.name == "a+1")


def full_batches():
    return [(kind, reqs * 3) for kind, reqs in case_batches(FULL_CASE) if kind != "raise"]


# whatif_copy_kernel's tile is 4,096 words: two tiles on the scalar path twice
# (N % 4 != 0), and the vector path with a last tile of one uint4
COPY_NODES = (4097, 4099, 4100)


def path_dbs(n):
    """The path 0 - 1 - ... - (n - 1) at metric 1, and a second link 0 - 1 at
    metric 3, which is on no shortest path."""
    adj = {v: [(u, 1) for u in (v - 1, v + 1) if 0 <= u < n] for v in range(n)}
    adj[0].append((1, 3))
    adj[1].append((0, 3))
    return int_topology(adj)


def copy_sources(n):
    return ["0", str(n // 2)]


def copy_requests(n):
    """8 requests on path_dbs(n) from copy_sources(n), four of them tier 0, as
    (source index, request, nodes, edges, tier under DEFAULT_CAPS). A cut
    path leaves what is behind the cut unreached. The cut at the middle node
    re-derives 2,048 nodes of the 4,097 (tier 2) and 2,049 of the others."""
    mid = n // 2
    spare = (link("0", "1", 1), 0, 0, 0)

    def cut(v):
        """Ignore v - (v + 1), from a source in front of it: v + 1 .. n - 1 are cut off."""
        nodes = n - 1 - v
        return (link(str(v), str(v + 1)), nodes, 2 * (nodes - 1), expected_tier(nodes, 2 * (nodes - 1), *DEFAULT_CAPS))
    picks = [(0, cut(n - 3)), (0, spare), (1, spare), (0, cut(1)), (1, cut(n - 2)), (0, spare), (1, cut(mid)),
             (1, spare)]
    return [(k, {"ignore": [key]}, nodes, edges, tier) for k, (key, nodes, edges, tier) in picks]
