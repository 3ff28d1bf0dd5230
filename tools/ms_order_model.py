#!/usr/bin/env python3
"""CPU model of what a node order costs the multi-source BFS (numpy only).

spf_msbfs_kernel pays per 64-node slice (a wave's nodes of one j: 64
consecutive device ids), not per node: the frontier gathers run for every
slice that still has a node short of a bit, and one log store instruction is
issued per (slice, level) with any arrival. For an all-sources sweep in
batches of 32 consecutive device ids this tool replays the search level by
level and prints, summed over the batches:

  levels      levels with an arrival, per batch (the loop runs one more, which finds nothing)
  events      (node, level) pairs with an arrival - the log's 8-byte records
  stores      (slice, level) pairs with an arrival - log store instructions
  open        (slice, level) pairs whose gathers run - slices not yet full

  tools/ms_order_model.py grid:100 cm cluster host
  tools/ms_order_model.py ring:2011:4 cluster

Orders: cm (Cuthill-McKee, order_nodes), cluster (ms_cluster_order,
csrc/host/ms_order.h - restated here; tests/test_ms_order.py holds the two
together), host (the ids as given).
"""
from __future__ import annotations

import random
import sys

import numpy as np

RUN = 64  # nodes per slice
BATCH = 32  # sources per batch (u32 masks)


def grid(n):
    """n x n grid, node id = row * n + col."""
    adj = [[] for _ in range(n * n)]
    for r in range(n):
        for c in range(n):
            for rr, cc in ((r, c + 1), (r, c - 1), (r - 1, c), (r + 1, c)):
                if 0 <= rr < n and 0 <= cc < n:
                    adj[r * n + c].append(rr * n + cc)
    return [sorted(a) for a in adj]


def ring_with_chords(n, k):
    """tests/test_gpu_msbfs_shapes.py's ring (seeded chords, one hub)."""
    rng = random.Random(1000 * n + k)
    base = 1 if k == 4 else 2
    adj = {v: [] for v in range(n)}

    def link(a, b):
        if a != b and b not in adj[a]:
            adj[a].append(b)
            adj[b].append(a)

    for v in range(n):
        for d in range(1, base + 1):
            link(v, (v + d) % n)
    cap = max(base + 1, n // 80)
    for _ in range(n // 8 if k == 4 else n // 3):
        a = rng.randrange(n)
        link(a, (a + rng.randint(base + 1, cap)) % n)
    hub = n // 2
    for d in range(1, 8):
        link(hub, hub + d)
        link(hub, hub - d)
    return [sorted(adj[v]) for v in range(n)]


def topology(spec):
    kind, *args = spec.split(":")
    if kind == "grid":
        return grid(int(args[0]))
    if kind == "ring":
        return ring_with_chords(int(args[0]), int(args[1]) if len(args) > 1 else 4)
    raise SystemExit(f"unknown topology {spec!r} (grid:N, ring:N[:K])")


def cm_order(adj):
    """order_nodes (orh_api.hip): BFS from a lowest-degree node of each
    component, neighbours in ascending degree, then id. Returns (host_of,
    depth): device id -> node, and the deepest BFS level of any component."""
    n = len(adj)
    deg = [len(a) for a in adj]
    dev_of = [-1] * n
    host_of = []
    level = [0] * n
    depth = 0
    for root in sorted(range(n), key=lambda v: deg[v]):  # stable
        if dev_of[root] >= 0:
            continue
        dev_of[root] = len(host_of)
        host_of.append(root)
        head = dev_of[root]
        while head < len(host_of):
            v = host_of[head]
            head += 1
            for u in sorted((u for u in adj[v] if dev_of[u] < 0), key=lambda u: deg[u]):
                dev_of[u] = len(host_of)
                level[u] = level[v] + 1
                depth = max(depth, level[u])
                host_of.append(u)
    return host_of, depth


def cluster_order(adj, cm_host_of):
    """ms_cluster_order (csrc/host/ms_order.h) restated: device ids in runs of
    64 that are compact BFS clusters. A cluster is seeded from the queue of
    unassigned nodes next to finished clusters (else the lowest unassigned
    Cuthill-McKee id: a new component) and grown by BFS over unassigned nodes,
    neighbours in Cuthill-McKee order, until its run of 64 ids is full. A
    growth that runs dry inside a component (a pocket between finished
    clusters) takes the next seed into the same run; a component's end leaves
    the run to be filled by the next component's first cluster."""
    n = len(adj)
    cm_of = [0] * n
    for d, v in enumerate(cm_host_of):
        cm_of[v] = d
    nbrs = [sorted(a, key=lambda u: cm_of[u]) for a in adj]
    dev_of = [-1] * n
    host_of = []
    seeds = []  # FIFO
    seed_head = 0
    next_cm = 0
    while len(host_of) < n:
        seed = -1
        while seed_head < len(seeds):
            s = seeds[seed_head]
            seed_head += 1
            if dev_of[s] < 0:
                seed = s
                break
        if seed < 0:
            while dev_of[cm_host_of[next_cm]] >= 0:
                next_cm += 1
            seed = cm_host_of[next_cm]
        first = len(host_of)
        room = RUN - first % RUN
        dev_of[seed] = first
        host_of.append(seed)
        head = first
        while head < len(host_of) and len(host_of) - first < room:
            v = host_of[head]
            head += 1
            for u in nbrs[v]:
                if dev_of[u] < 0:
                    dev_of[u] = len(host_of)
                    host_of.append(u)
                    if len(host_of) - first == room:
                        break
        for v in host_of[first:]:
            for u in nbrs[v]:
                if dev_of[u] < 0:
                    seeds.append(u)
    return host_of


def model(adj, host_of):
    """Replays the all-sources sweep; returns (batches, levels, events, stores, open)."""
    n = len(adj)
    dev_of = np.empty(n, dtype=np.int64)
    dev_of[np.asarray(host_of)] = np.arange(n)
    kmax = max(1, max(len(a) for a in adj))
    nbr = np.full((n, kmax), n, dtype=np.int64)  # n: the always-zero entry
    for v, a in enumerate(adj):
        nbr[dev_of[v], : len(a)] = dev_of[np.asarray(a, dtype=np.int64)] if a else []
    starts = np.arange(0, n, RUN)
    batches = levels = events = stores = opened = 0
    for b0 in range(0, n, BATCH):
        s = min(BATCH, n - b0)
        full = np.uint32((1 << s) - 1 if s < 32 else 0xFFFFFFFF)
        vis = np.zeros(n, dtype=np.uint32)
        vis[b0 : b0 + s] = np.uint32(1) << np.arange(s, dtype=np.uint32)
        f = np.zeros(n + 1, dtype=np.uint32)
        f[:n] = vis
        arrived = vis != 0
        events += int(arrived.sum())
        stores += int(np.add.reduceat(arrived, starts).astype(bool).sum())
        batches += 1
        while True:
            short = vis != full
            opened += int(np.add.reduceat(short, starts).astype(bool).sum())
            nx = np.bitwise_or.reduce(f[nbr], axis=1) & ~vis
            arrived = nx != 0
            k = int(arrived.sum())
            if not k:
                break
            levels += 1
            vis |= nx
            events += k
            stores += int(np.add.reduceat(arrived, starts).astype(bool).sum())
            f[:n] = nx
    return batches, levels, events, stores, opened


def main(argv):
    if len(argv) < 3:
        raise SystemExit(__doc__)
    adj = topology(argv[1])
    n = len(adj)
    cm, depth = cm_order(adj)
    print(f"{argv[1]}: {n} nodes, Cuthill-McKee BFS depth {depth}; 512 threads' slices of {RUN}, batches of {BATCH}")
    print(f"{'order':8s} {'levels/batch':>12s} {'events':>12s} {'/node':>6s} {'stores':>10s} {'open':>10s}")
    for name in argv[2:]:
        if name == "cm":
            order = cm
        elif name == "cluster":
            order = cluster_order(adj, cm)
        elif name == "host":
            order = list(range(n))
        else:
            raise SystemExit(f"unknown order {name!r}")
        assert sorted(order) == list(range(n))
        b, lv, ev, stc, op = model(adj, order)
        print(f"{name:8s} {lv / b:12.1f} {ev:12d} {ev / (b * n):6.2f} {stc:10d} {op:10d}", flush=True)


if __name__ == "__main__":
    main(sys.argv)
