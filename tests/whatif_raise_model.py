"""Pure-Python statement of the what-if repair rule with metric raises
(whatif_kernels.hip, orh_whatif_run_metrics), and the helpers the raise tests
share.

A request changes its source's plain SPF row by ignoring links, draining nodes
(treating them as overloaded) and raising the metric one end of a link
advertises. All three only weaken relaxations, so the row changes only on the
affected set A and is re-derived there:

  cuts      both records of an ignored link, every out-record of a drained
            node (never the source), every raised record
  seeds     heads of the cuts that are tight in the base row under the record's
            own, OLD weight, with a tail that is reached and is the source or
            not overloaded
  closure   A grows along records tight under the old weights out of nodes
            that are neither overloaded nor drained
  labels    for v in A the lattice meet (smaller distance replaces, equal
            distance unites the first-hop sets) over its in-records p -> v: an
            ignored link is skipped, so is an overloaded or drained p other
            than the source; the record weighs its raised value if the request
            has one, else its own. p outside A offers its base label, p inside
            A its current one, until nothing changes.

Rows are {node: (distance, sorted first-hop names)}, unreached nodes absent:
the form of the oracle's run_spf_ignoring.
"""
import collections
import dataclasses
import heapq

Rec = collections.namedtuple("Rec", "tail head key w")


def link_key(desc):
    """A link descriptor (n1, if1, n2, if2) whichever end comes first."""
    return tuple(sorted(((desc[0], desc[1]), (desc[2], desc[3]))))


class Graph:
    """The up links of a list of adjacency databases as directed records (one
    per link and direction, with the metric its tail advertises), the down
    links' keys, and the overloaded nodes."""

    def __init__(self, dbs):
        self.nodes = sorted(db.thisNodeName for db in dbs)
        self.overloaded = {db.thisNodeName for db in dbs if db.isOverloaded}
        adj = {(db.thisNodeName, a.ifName): a for db in dbs for a in db.adjacencies}
        self.out = {x: [] for x in self.nodes}
        self.into = {x: [] for x in self.nodes}
        self.metric = {}  # (key, tail) -> advertised metric, down links included
        self.down = set()
        for (x, i), a in sorted(adj.items()):
            b = adj.get((a.otherNodeName, a.otherIfName))
            if b is None or b.otherNodeName != x or b.otherIfName != i:
                continue  # half a link
            key = link_key((x, i, a.otherNodeName, a.otherIfName))
            self.metric[(key, x)] = a.metric
            if a.isOverloaded or b.isOverloaded:
                self.down.add(key)
                continue
            rec = Rec(x, a.otherNodeName, key, a.metric)
            self.out[x].append(rec)
            self.into[a.otherNodeName].append(rec)

    def ends(self, key):
        return [key[0][0], key[1][0]]


def effective_raises(graph, raises):
    """[(key, end or None, metric)] -> {(key, tail): metric}: both ends for
    None, the largest of a repeated (link, end), raises to the current value
    and raises of down links dropped; a decrease is a ValueError."""
    out = {}
    for key, end, metric in raises:
        for tail in (graph.ends(key) if end is None else [end]):
            cur = graph.metric[(key, tail)]
            if metric < cur:
                raise ValueError("metric decrease")
            if metric > cur and key not in graph.down:
                out[(key, tail)] = max(metric, out.get((key, tail), 0))
    return out


def raised_dbs(dbs, eff, drain=()):
    """The databases with the metrics of effective_raises replaced on the
    Adjacency of the raising end, and isOverloaded set on the drained nodes."""
    out = []
    for db in dbs:
        x = db.thisNodeName
        adjs = []
        for a in db.adjacencies:
            key = link_key((x, a.ifName, a.otherNodeName, a.otherIfName))
            m = eff.get((key, x))
            adjs.append(dataclasses.replace(a, metric=m) if m is not None else a)
        out.append(dataclasses.replace(db, adjacencies=adjs, isOverloaded=db.isOverloaded or x in drain))
    return out


def _meet(label, d, hops):
    if d < label[0]:
        return (d, frozenset(hops))
    if d == label[0]:
        return (d, label[1] | hops)
    return label


def spf(graph, src):
    """The plain row as {node: (dist, frozenset of first hops)}."""
    dist = {src: 0}
    heap = [(0, src)]
    while heap:
        d, x = heapq.heappop(heap)
        if d > dist[x] or (x != src and x in graph.overloaded):
            continue
        for r in graph.out[x]:
            if d + r.w < dist.get(r.head, float("inf")):
                dist[r.head] = d + r.w
                heapq.heappush(heap, (d + r.w, r.head))
    row = {src: (0, frozenset())}
    for v in sorted((v for v in dist if v != src), key=dist.get):  # positive metrics
        hops = frozenset()
        for r in graph.into[v]:
            p = r.tail
            if p in row and (p == src or p not in graph.overloaded) and dist[p] + r.w == dist[v]:
                hops |= frozenset([v]) if p == src else row[p][1]
        row[v] = (dist[v], hops)
    return row


def repair(graph, src, base, ignore=(), drain=(), eff=None):
    """The request's row derived from `base` (spf(graph, src)) by the rule in
    the module docstring, and its affected set. ignore: link keys; drain: node
    names; eff: effective_raises."""
    eff = eff or {}
    ignore = set(ignore)
    drain = set(drain) - {src}
    inf = float("inf")

    def d(x):
        return base[x][0] if x in base else inf

    cuts = [r for x in graph.nodes for r in graph.out[x]
            if r.key in ignore or x in drain or (r.key, x) in eff]
    seeds = {r.head for r in cuts
             if d(r.tail) != inf and (r.tail == src or r.tail not in graph.overloaded) and d(r.tail) + r.w == d(r.head)}
    affected, level = set(seeds), list(seeds)
    while level:
        nxt = []
        for v in level:
            if v in graph.overloaded or v in drain:
                continue
            for r in graph.out[v]:
                if r.head not in affected and d(v) + r.w == d(r.head):  # the old weight
                    affected.add(r.head)
                    nxt.append(r.head)
        level = nxt
    assert src not in affected

    def preds(v):
        for r in graph.into[v]:
            p = r.tail
            if r.key in ignore or (p != src and (p in graph.overloaded or p in drain)):
                continue
            yield p, eff.get((r.key, p), r.w)

    none = (inf, frozenset())
    boundary, inside = {}, {}
    for v in affected:
        label, edges = none, []
        for p, w in preds(v):
            if p in affected:
                edges.append((p, w))
            elif d(p) != inf:
                label = _meet(label, d(p) + w, frozenset([v]) if p == src else base[p][1])
        boundary[v], inside[v] = label, edges
    lab = {v: none for v in affected}
    changed = True
    while changed:
        changed = False
        for v in sorted(affected):
            new = boundary[v]
            for p, w in inside[v]:
                if lab[p][0] != inf:
                    new = _meet(new, lab[p][0] + w, lab[p][1])
            if new != lab[v]:
                lab[v], changed = new, True
    row = {v: l for v, l in base.items() if v not in affected}
    row.update({v: l for v, l in lab.items() if l[0] != inf})
    return row, affected


def view(row):
    """A model row in run_spf_ignoring's form."""
    return {v: (dist, sorted(hops)) for v, (dist, hops) in row.items()}
