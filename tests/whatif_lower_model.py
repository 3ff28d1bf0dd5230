"""Pure-Python statement of the two-stage rule for what-if requests that lower
link metrics (whatif_lower_kernels.hip, orh_whatif_run_lowers), and the helpers
the lower tests share.

Stage 1 is whatif_raise_model.repair: the request's ignored links, drained
nodes and raises, which leave the row R1. Stage 2 turns R1 into the row of the
graph with the lowered metrics as well. "Transit": the node is the source, or
neither overloaded nor drained. An ignored link is skipped everywhere. A record
weighs its lowered value if the request lowers it, else its raised value, else
its own weight.

  distances  seeds: heads v of lowered records p -> v, p reached and transit,
             d(p) + w' < d(v); then a label-correcting wave: a node whose
             distance fell relaxes its out-records if it is transit. C = the
             nodes whose distance fell.
  mask set   M = C plus the heads of lowered records now tight (p reached and
             transit), closed under records tight in the NEW distances and
             weights out of transit nodes.
  labels     for v in M the first hops are the union over its tight
             predecessors: the source offers v itself, a predecessor outside M
             its R1 set, one inside M its current set; from empty sets until
             nothing changes.

Rows are {node: (distance, frozenset of first hops)} as in
whatif_raise_model.
"""
import dataclasses

from whatif_raise_model import link_key, repair


def effective_lowers(graph, lowers):
    """[(key, end or None, metric)] -> {(key, tail): metric}: both ends for
    None, the smallest of a repeated (link, end), lowers to the current value
    and lowers of down links dropped; an increase or a zero is a ValueError."""
    out = {}
    for key, end, metric in lowers:
        if key in graph.down:
            continue
        if metric == 0:
            raise ValueError("zero metric")
        tails = graph.ends(key) if end is None else [end]
        if any(metric > graph.metric[(key, t)] for t in tails):
            raise ValueError("metric increase")
        for tail in tails:
            if metric < graph.metric[(key, tail)]:
                out[(key, tail)] = min(metric, out.get((key, tail), metric))
    return out


def changed_dbs(dbs, eff_raise, eff_lower, drain=()):
    """The databases with the raised and the lowered metrics replaced on the
    Adjacency of the changing end, and isOverloaded set on the drained nodes."""
    assert not set(eff_raise) & set(eff_lower)
    eff = {**eff_raise, **eff_lower}
    out = []
    for db in dbs:
        x = db.thisNodeName
        adjs = []
        for a in db.adjacencies:
            m = eff.get((link_key((x, a.ifName, a.otherNodeName, a.otherIfName)), x))
            adjs.append(dataclasses.replace(a, metric=m) if m is not None else a)
        out.append(dataclasses.replace(db, adjacencies=adjs, isOverloaded=db.isOverloaded or x in drain))
    return out


def lower(graph, src, r1, ignore=(), drain=(), eff_raise=None, eff_lower=None):
    """Stage 2: the row of the graph with the lowered metrics from R1, and M."""
    eff_raise, eff_lower = eff_raise or {}, eff_lower or {}
    ignore = set(ignore)
    drain = set(drain) - {src}
    inf = float("inf")
    dist = {v: l[0] for v, l in r1.items()}

    def d(x):
        return dist.get(x, inf)

    def transit(x):
        return x == src or (x not in graph.overloaded and x not in drain)

    def weight(r):
        return eff_lower.get((r.key, r.tail), eff_raise.get((r.key, r.tail), r.w))

    lowered = [r for x in graph.nodes for r in graph.out[x] if (r.key, x) in eff_lower and r.key not in ignore]
    # distances
    fell, work = set(), []
    for r in lowered:
        if d(r.tail) != inf and transit(r.tail) and d(r.tail) + weight(r) < d(r.head):
            dist[r.head] = d(r.tail) + weight(r)
            fell.add(r.head)
            work.append(r.head)
    while work:
        v = work.pop()
        if not transit(v):
            continue
        for r in graph.out[v]:
            if r.key not in ignore and d(v) + weight(r) < d(r.head):
                dist[r.head] = d(v) + weight(r)
                fell.add(r.head)
                work.append(r.head)
    # mask set
    m = set(fell) | {r.head for r in lowered
                     if d(r.tail) != inf and transit(r.tail) and d(r.tail) + weight(r) == d(r.head)}
    level = list(m)
    while level:
        nxt = []
        for v in level:
            if not transit(v):
                continue
            for r in graph.out[v]:
                if r.key not in ignore and r.head not in m and d(v) + weight(r) == d(r.head):
                    m.add(r.head)
                    nxt.append(r.head)
        level = nxt
    assert src not in m
    # labels
    hops = {v: frozenset() for v in m}
    changed = True
    while changed:
        changed = False
        for v in sorted(m):
            new = frozenset()
            for r in graph.into[v]:
                p = r.tail
                if r.key in ignore or not transit(p) or d(p) == inf or d(p) + weight(r) != d(v):
                    continue
                new |= frozenset([v]) if p == src else hops[p] if p in m else r1[p][1]
            if new != hops[v]:
                hops[v], changed = new, True
    row = {v: l for v, l in r1.items() if v not in m}
    row.update({v: (dist[v], hops[v]) for v in m})
    return row, m


def two_stage(graph, src, base, ignore=(), drain=(), eff_raise=None, eff_lower=None):
    """Both stages from the plain row: (row, stage 1's affected set, M)."""
    r1, affected = repair(graph, src, base, ignore, drain, eff_raise)
    row, m = lower(graph, src, r1, ignore, drain, eff_raise, eff_lower)
    return row, affected, m


def request_families(graph, rng, n_srcs, mixed=40):
    """The requests the model test and the GPU test share, as (source index,
    ignored keys, drained nodes, raises, lowers) with raises and lowers as
    (key, end or None, metric), and the half-open ranges of the families:

      single   every link lowered from each end and from both, to cur - 1,
               (cur + 1) // 2 and 1 (where those are below cur), per source
      same     every link lowered to the current value from one end: dropped
      sets     2-3 lowers
      ignore   a lower and an ignored link (any link)
      drain    a lower and a drained node
      raise    a lower and a raise of another link
      thrice   the same (link, end) three times: the smallest holds
      ignored  a link both lowered and ignored: ignored
    """
    keys = sorted({k for k, _ in graph.metric})

    def cur(key, end):
        return min(graph.metric[(key, t)] for t in (graph.ends(key) if end is None else [end]))

    def some_lower(but=None):
        for _ in range(1000):
            key = rng.choice([k for k in keys if k != but])
            end = rng.choice(graph.ends(key) + [None])
            c = cur(key, end)
            if c > 1:
                return (key, end, rng.choice(sorted({c - 1, (c + 1) // 2, 1})))
        raise AssertionError("no link to lower")

    reqs, marks = [], {}

    def family(name, items):
        lo = len(reqs)
        reqs.extend(items)
        marks[name] = (lo, len(reqs))

    family("single", [(k, [], [], [], [(key, end, value)])
                      for key in keys for end in graph.ends(key) + [None]
                      for value in sorted({cur(key, end) - 1, (cur(key, end) + 1) // 2, 1} - {0, cur(key, end)})
                      for k in range(n_srcs)])
    family("same", [(rng.randrange(n_srcs), [], [], [], [(key, end, cur(key, end))])
                    for key in keys for end in [rng.choice(graph.ends(key))]])
    family("sets", [(rng.randrange(n_srcs), [], [], [], [some_lower() for _ in range(rng.choice((2, 3)))])
                    for _ in range(mixed)])
    family("ignore", [(rng.randrange(n_srcs), [rng.choice(keys)], [], [], [some_lower()]) for _ in range(mixed)])
    family("drain", [(rng.randrange(n_srcs), [], [rng.choice(graph.nodes)], [], [some_lower()])
                     for _ in range(mixed)])
    items = []
    for _ in range(mixed):
        low = some_lower()
        key = rng.choice([k for k in keys if k != low[0]])
        end = rng.choice(graph.ends(key) + [None])
        top = max(graph.metric[(key, t)] for t in graph.ends(key))
        items.append((rng.randrange(n_srcs), [], [], [(key, end, rng.choice((top + 1, top * 3, 10 ** 6)))], [low]))
    family("raise", items)
    items = []
    for _ in range(mixed):
        key, end, value = some_lower()
        c = cur(key, end)
        items.append((rng.randrange(n_srcs), [], [], [], [(key, end, min(value + 2, c)), (key, end, value),
                                                        (key, end, min(value + 1, c))]))
    family("thrice", items)
    family("ignored", [(rng.randrange(n_srcs), [low[0]], [], [], [low]) for low in (some_lower() for _ in range(mixed))])
    return reqs, marks
