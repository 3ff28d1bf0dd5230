"""Benchmark workloads of BASELINE.json's configs.

  C1  createGrid(10, 1 prefix, SP_ECMP)                      topology.bench_grid(10)
  C2  createGrid(100): all-sources SPF                       topology.bench_grid(100)
  C3  3-tier Clos of ~2.5k nodes (full spine mesh) + 100k /64s over the
      RSWs (~54 each) and a seeded 5% anycast subset (2-8 advertisers),
      default and best-route selection                       c3_fabric()
  C3w the same Clos with seeded metrics 1..64: weighted all-sources sweep
      of a high-degree graph (tools/c3w_sweep.py)            c3_weighted_fabric()
  C4  50k-node WAN, log-normal metrics: single-link what-if SPFs and KSP2
      (src, dst) pairs                                       c4_wan()
  C5  4 areas x ~2.5k nodes, myNode in all four, 1M prefixes with random
      PrefixMetrics, best-route selection, RibPolicy area weights
                                                             c5_multi_area()
All seeded; nothing is read from disk.
"""
from __future__ import annotations

import random
from typing import List, Tuple

from .topology import _hex2, bench_grid, fabric, wan
from .types import (K_TESTING_AREA, Adjacency, BinaryAddress, IpPrefix, PrefixEntry,
                    PrefixMetrics, PrefixType, create_adj_db)

C3_SEED, C4_SEED, C5_SEED = 3003, 4004, 5005
# C4 batch shape (SURVEY.md §8d / BASELINE.md): 4,096 sampled links x 64
# sources of runSpf(src, true, {link}), and 1,024 KSP2 (src, dst) pairs
C4_WHATIF_LINKS, C4_WHATIF_SRCS, C4_KSP2_PAIRS = 4096, 64, 1024
# requests per what-if run: two alternating device row buffers of
# CHUNK x N x 8 bytes (2 x 26 GB at N = 50,000 of the 288 GB HBM), so the
# large repairs of one chunk overlap the next chunk's copy
C4_WHATIF_CHUNK = 65536


def _metrics(rng):
    return PrefixMetrics(1, rng.randint(0, 3), rng.randint(0, 3), rng.randint(0, 3))


def c3_fabric(num_nodes: int = 2500, num_prefixes: int = 100_000, anycast: float = 0.05,
              seed: int = C3_SEED, area: str = K_TESTING_AREA):
    """Full-mesh Clos (N = 2,472 at 2,500) + prefixes (node, area, entry)."""
    adj_dbs, _ = fabric(num_nodes, bug_compatible=False, area=area)
    rsws = [db.thisNodeName for db in adj_dbs if db.thisNodeName.startswith("3-")]
    rng = random.Random(seed)
    prefixes = []
    for i in range(num_prefixes):
        addr = BinaryAddress(bytes([0xfd, 0x00, (i >> 24) & 255, (i >> 16) & 255,
                                    (i >> 8) & 255, i & 255, 0, 0] + [0] * 8))
        p = IpPrefix(addr, 64)
        if rng.random() < anycast:
            owners = rng.sample(rsws, rng.randint(2, 8))
        else:
            owners = [rsws[i % len(rsws)]]
        for o in owners:
            prefixes.append((o, area, PrefixEntry(p, PrefixType.LOOPBACK,
                                                  metrics=_metrics(rng))))
    return adj_dbs, prefixes


C2W_SEED, C2W_MAX_METRIC = 2002, 64


def c2_weighted_grid(n: int = 100, max_metric: int = C2W_MAX_METRIC, seed: int = C2W_SEED):
    """C2 with integer metrics (the weighted all-sources leg): the benchmark
    grid createGrid(n) (topology.bench_grid) with every link given a seeded
    metric uniform in [1, max_metric], the same in both directions (an IGP
    cost per link). Returns (adj_dbs, prefixes) like bench_grid."""
    adj_dbs, prefixes = bench_grid(n, 1)
    rng = random.Random(seed)
    metric = {}
    for db in adj_dbs:
        a = int(db.thisNodeName)
        for adj in db.adjacencies:
            b = int(adj.otherNodeName)
            key = (min(a, b), max(a, b))
            if key not in metric:
                metric[key] = rng.randint(1, max_metric)
            adj.metric = metric[key]
    return adj_dbs, prefixes


C3W_SEED, C3W_MAX_METRIC = 3303, 64


def weight_links(adj_dbs, lo: int, hi: int, seed: int, symmetric: bool = True):
    """Give every adjacency a seeded metric uniform in [lo, hi], drawn in
    adjacency order: one draw per link (its first appearance), the same in
    both directions, when ``symmetric``; else one draw per direction."""
    rng = random.Random(seed)
    metric = {}
    for db in adj_dbs:
        a = db.thisNodeName
        for adj in db.adjacencies:
            if not symmetric:
                adj.metric = rng.randint(lo, hi)
                continue
            b = adj.otherNodeName
            key = (min(a, b), max(a, b))
            if key not in metric:
                metric[key] = rng.randint(lo, hi)
            adj.metric = metric[key]
    return adj_dbs


def c3_weighted_fabric(num_nodes: int = 2500, max_metric: int = C3W_MAX_METRIC, seed: int = C3W_SEED,
                       symmetric: bool = True, area: str = K_TESTING_AREA):
    """C3's Clos with integer metrics (the weighted all-sources sweep of a
    high-degree graph: spines of degree 39, FSWs of 84, RSWs of 8 at 2,500):
    fabric(num_nodes, bug_compatible=False) with every link given a seeded
    metric uniform in [1, max_metric] (weight_links). Returns (adj_dbs,
    prefixes) like fabric."""
    adj_dbs, prefixes = fabric(num_nodes, bug_compatible=False, area=area)
    return weight_links(adj_dbs, 1, max_metric, seed, symmetric), prefixes


def c4_wan(num_nodes: int = 50_000, seed: int = C4_SEED):
    return wan(num_nodes, seed=seed)


def c4_what_if_pairs(link_ids: List[int], node_names: List[str], n_links: int, n_srcs: int,
                     seed: int = C4_SEED) -> List[Tuple[str, int]]:
    """(source, ignored link) pairs: n_links sampled links x n_srcs sampled sources."""
    rng = random.Random(seed + 1)
    links = rng.sample(link_ids, min(n_links, len(link_ids)))
    srcs = rng.sample(node_names, min(n_srcs, len(node_names)))
    return [(s, l) for l in links for s in srcs]


def c4_what_if_job(link_ids: List[int], node_names: List[str], n_links: int = C4_WHATIF_LINKS,
                   n_srcs: int = C4_WHATIF_SRCS, seed: int = C4_SEED):
    """The same (source, link) requests as c4_what_if_pairs, as a what-if job:
    (sources, per request its source index, per request its ignore set)."""
    rng = random.Random(seed + 1)
    links = rng.sample(link_ids, min(n_links, len(link_ids)))
    srcs = rng.sample(node_names, min(n_srcs, len(node_names)))
    idx = [i for _ in links for i in range(len(srcs))]
    sets = [[l] for l in links for _ in srcs]
    return srcs, idx, sets


def c4_drain_job(node_names: List[str], n_nodes: int = C4_WHATIF_LINKS, n_srcs: int = C4_WHATIF_SRCS,
                 seed: int = C4_SEED):
    """The drain analogue of c4_what_if_job: "what if this node is drained?"
    for n_nodes seeded nodes x n_srcs seeded sources. Returns (sources, per
    request its source index, per request its (empty) ignore set, per request
    its drained node names); the requests are in the link job's order, the
    drained node outermost, one node each."""
    rng = random.Random(seed + 3)
    nodes = rng.sample(node_names, min(n_nodes, len(node_names)))
    srcs = rng.sample(node_names, min(n_srcs, len(node_names)))
    idx = [i for _ in nodes for i in range(len(srcs))]
    ignore = [[] for _ in nodes for _ in srcs]
    drain = [[x] for x in nodes for _ in srcs]
    return srcs, idx, ignore, drain


def c4_costout_job(links, adj_dbs, node_names: List[str], n_links: int = C4_WHATIF_LINKS,
                   n_srcs: int = C4_WHATIF_SRCS, factor: int = 10, seed: int = C4_SEED):
    """The cost-out analogue of c4_what_if_job: "where does traffic go if this
    link's metric is raised x factor from both ends?" for the link job's links
    and sources. links: (link id, (node1, if1, node2, if2)) pairs as
    LinkState.link_ids() gives them; adj_dbs: the loaded adjacency databases
    (each end's current metric). Returns (sources, per request its source
    index, per request its (empty) ignore set, per request its raises
    [(link id, end name, new metric)] - one per end, each end's own metric
    times factor)."""
    desc = dict(links)
    srcs, idx, sets = c4_what_if_job([lid for lid, _ in links], node_names, n_links, n_srcs, seed)
    cur = {(db.thisNodeName, a.ifName): a.metric for db in adj_dbs for a in db.adjacencies}
    ignore = [[] for _ in sets]
    metric = []
    for (lid,) in sets:
        n1, if1, n2, if2 = desc[lid]
        metric.append([(lid, n1, cur[(n1, if1)] * factor), (lid, n2, cur[(n2, if2)] * factor)])
    return srcs, idx, ignore, metric


def c4_costin_job(links, adj_dbs, node_names: List[str], n_links: int = C4_WHATIF_LINKS,
                  n_srcs: int = C4_WHATIF_SRCS, factor: int = 10, seed: int = C4_SEED):
    """The cost-in twin of c4_costout_job: the link job's links are costed
    out (both ends' metrics x factor) in the graph itself, and request (link,
    source) asks "what changes if this link is costed back in?" by lowering
    both ends to their plain values. links, adj_dbs as for c4_costout_job (the
    plain graph). Returns (the costed-out adjacency databases to load - same
    structure, so the same link ids -, sources, per request its source index,
    per request its (empty) ignore set, per request its lowers [(link id, end
    name, plain metric)] - one per end)."""
    import dataclasses
    desc = dict(links)
    srcs, idx, sets = c4_what_if_job([lid for lid, _ in links], node_names, n_links, n_srcs, seed)
    cur = {(db.thisNodeName, a.ifName): a.metric for db in adj_dbs for a in db.adjacencies}
    costed = set()
    for lid in {l for (l,) in sets}:
        n1, if1, n2, if2 = desc[lid]
        costed.update(((n1, if1), (n2, if2)))
    dbs = [dataclasses.replace(db, adjacencies=[
        dataclasses.replace(a, metric=a.metric * factor) if (db.thisNodeName, a.ifName) in costed else a
        for a in db.adjacencies]) for db in adj_dbs]
    ignore = [[] for _ in sets]
    lower = []
    for (lid,) in sets:
        n1, if1, n2, if2 = desc[lid]
        lower.append([(lid, n1, cur[(n1, if1)]), (lid, n2, cur[(n2, if2)])])
    return dbs, srcs, idx, ignore, lower


def c4_node_weights(node_names: List[str], seed: int = C4_SEED, max_prefixes: int = 64):
    """Seeded per-node weights for what-if impact summaries on the C4 WAN: the
    prefixes each node advertises, uniform in [0, max_prefixes], as
    {node name: weight}."""
    rng = random.Random(seed + 4)
    return {x: rng.randint(0, max_prefixes) for x in node_names}


def c4_ksp2_pairs(node_names: List[str], n_pairs: int, seed: int = C4_SEED):
    rng = random.Random(seed + 2)
    out = []
    while len(out) < n_pairs:
        a, b = rng.sample(node_names, 2)
        out.append((a, b))
    return out


C5_AREAS = ("A", "B", "C", "D")
C5_TAG = "C5:UCMP"  # every C5 prefix carries it; the RibPolicy statement matches on it


def c5_multi_area(side: int = 50, num_prefixes: int = 1_000_000, seed: int = C5_SEED,
                  me: str = "me"):
    """Four grid areas of side x side nodes (2,500 at side 50); `me` is in all
    four, attached to one corner node of each grid (metric 1). Prefixes are
    /64s spread over all nodes with random PrefixMetrics; 5% anycast across
    areas. Returns ({area: adj_dbs}, prefixes)."""
    rng = random.Random(seed)
    areas = {}
    names_by_area = {}
    for ai, area in enumerate(C5_AREAS):
        dbs, _ = bench_grid(side, 0, area=area)
        # rename nodes per area so areas do not share node names (except me)
        ren = {db.thisNodeName: f"{area}{db.thisNodeName}" for db in dbs}
        for db in dbs:
            db.thisNodeName = ren[db.thisNodeName]
            for adj in db.adjacencies:
                adj.otherNodeName = ren[adj.otherNodeName]
            db.nodeLabel = (ai + 1) * 10000 + db.nodeLabel
        corner = dbs[0]
        up = Adjacency(corner.thisNodeName, f"me-{area}", BinaryAddress.of(f"fe80::{ai + 1}:1"),
                       BinaryAddress.of(f"10.250.{ai}.1"), 1, 0, False, 100, 10000, 1,
                       f"{corner.thisNodeName}-me")
        down = Adjacency(me, f"{corner.thisNodeName}-me", BinaryAddress.of(f"fe80::{ai + 1}:2"),
                         BinaryAddress.of(f"10.250.{ai}.2"), 1, 0, False, 100, 10000, 1,
                         f"me-{area}")
        corner.adjacencies.append(down)
        dbs.append(create_adj_db(me, [up], 1, False, area))
        areas[area] = dbs
        names_by_area[area] = [db.thisNodeName for db in dbs if db.thisNodeName != me]
    prefixes = []
    for i in range(num_prefixes):
        addr = BinaryAddress(bytes([0xfc, 0x05, (i >> 24) & 255, (i >> 16) & 255,
                                    (i >> 8) & 255, i & 255, 0, 0] + [0] * 8))
        p = IpPrefix(addr, 64)
        if rng.random() < 0.05:
            owners = [(a, rng.choice(names_by_area[a])) for a in rng.sample(C5_AREAS, 2)]
        else:
            a = C5_AREAS[i % 4]
            owners = [(a, names_by_area[a][(i // 4) % len(names_by_area[a])])]
        for a, o in owners:
            prefixes.append((o, a, PrefixEntry(p, metrics=_metrics(rng), tags=(C5_TAG,))))
    return areas, prefixes
