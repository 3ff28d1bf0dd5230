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

and what the adjacency skip (kMsSkipAdj; slice_adjacency below restates
ms_slice_adjacency of csrc/host/ms_order.h) leaves of that. A slice is todo
at level L when a slice adjacent to it, or itself, had an arrival at level
L - 1 (level 0: the sources' slices); no arrival ever falls outside the todo
slices (asserted on every level):

  need        open slices that are todo
  open_g      groups of 2 slices of a wave (slices j * waves + w and
              (j + 1) * waves + w, j even) with an open slice: what runs today
  need_g      groups with an open slice and a todo slice: the kernel's exact
              run condition
  crit        groups run by the busiest wave, summed over the batch-levels
              (what the level barrier waits for), without / with the skip,
              and the same per level

The workgroup is plan_spf's: 256 threads up to 4,096 nodes, 512 up to 16,384.

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


def _ceil(a, b):
    return -(-a // b)


def slice_adjacency(adj, host_of):
    """ms_slice_adjacency (csrc/host/ms_order.h) restated: per 64-id slice of
    the order, the ascending list of the slices that hold a neighbour of any
    of its nodes, the slice itself included."""
    n = len(adj)
    dev_of = [0] * n
    for d, v in enumerate(host_of):
        dev_of[v] = d
    sets = [{s} for s in range((n + RUN - 1) // RUN)]
    for v, a in enumerate(adj):
        sets[dev_of[v] // RUN].update(dev_of[u] // RUN for u in a)
    return [sorted(x) for x in sets]


def plan_waves(n):
    """Waves per workgroup of plan_spf's multi-source BFS shape."""
    return 4 if n <= 4096 else 8 if n <= 16384 else 12


def model(adj, host_of):
    """Replays the all-sources sweep; returns (batches, levels, events, stores, open)."""
    r = replay(adj, host_of)
    return r["batches"], r["levels"], r["events"], r["stores"], r["open"]


def replay(adj, host_of, sadj=None, waves=None):
    """Replays the all-sources sweep with the adjacency skip's bookkeeping
    (sadj: the slice adjacency, default slice_adjacency's; waves: per
    workgroup, default plan_waves'). Returns the columns by name."""
    n = len(adj)
    sadj = slice_adjacency(adj, host_of) if sadj is None else sadj
    waves = plan_waves(n) if waves is None else waves
    n_sl = (n + RUN - 1) // RUN
    assert len(sadj) == n_sl
    jn = 4 * _ceil(_ceil(n, RUN * waves), 4)  # nodes per thread (plan_spf)
    amat = np.zeros((n_sl, n_sl), dtype=np.int32)
    for t, lst in enumerate(sadj):
        amat[t, lst] = 1

    def grouped(x):  # per slice -> per (group, wave): any of the group's 2 slices
        pad = np.zeros(jn * waves, dtype=bool)
        pad[:n_sl] = x
        return pad.reshape(jn // 2, 2, waves).any(axis=1)

    need = open_g = need_g = crit_open = crit_need = arrive = 0
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
        marked = np.add.reduceat(arrived, starts).astype(bool)  # level 0: the sources' slices
        stores += int(marked.sum())
        batches += 1
        while True:
            short = vis != full
            open_s = np.add.reduceat(short, starts).astype(bool)
            opened += int(open_s.sum())
            todo = amat @ marked.astype(np.int32) > 0
            need += int((open_s & todo).sum())
            og, tg = grouped(open_s), grouped(todo)
            open_g += int(og.sum())
            need_g += int((og & tg).sum())
            crit_open += int(og.sum(axis=0).max())
            crit_need += int((og & tg).sum(axis=0).max())
            nx = np.bitwise_or.reduce(f[nbr], axis=1) & ~vis
            arrived = nx != 0
            k = int(arrived.sum())
            marked = np.add.reduceat(arrived, starts).astype(bool)
            assert not (marked & ~todo).any(), "an arrival outside the todo slices"
            if not k:
                break
            levels += 1
            vis |= nx
            events += k
            stores += int(marked.sum())
            arrive += int(marked.sum())
            f[:n] = nx
    return {"batches": batches, "levels": levels, "events": events, "stores": stores, "open": opened,
            "need": need, "arrive": arrive, "open_g": open_g, "need_g": need_g, "crit_open": crit_open,
            "crit_need": crit_need, "waves": waves, "j": jn}


def main(argv):
    if len(argv) < 3:
        raise SystemExit(__doc__)
    adj = topology(argv[1])
    n = len(adj)
    cm, depth = cm_order(adj)
    print(f"{argv[1]}: {n} nodes, Cuthill-McKee BFS depth {depth}; slices of {RUN}, batches of {BATCH}, "
          f"{plan_waves(n)} waves a workgroup")
    print(f"{'order':8s} {'levels/batch':>12s} {'events':>12s} {'/node':>6s} {'stores':>10s} {'open':>10s}"
          f" {'need':>10s} {'open_g':>10s} {'need_g':>10s} {'crit':>17s} {'/level':>11s} {'adj/slice':>10s}")
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
        sadj = slice_adjacency(adj, order)
        r = replay(adj, order, sadj)
        b, lv, ev, stc, op = r["batches"], r["levels"], r["events"], r["stores"], r["open"]
        bl = lv + b  # batch-levels the loop runs: one more per batch, which finds nothing
        crit = f"{r['crit_open']}/{r['crit_need']}"
        per = f"{r['crit_open'] / bl:.1f}/{r['crit_need'] / bl:.1f}"
        deg = f"{sum(map(len, sadj)) / len(sadj):.1f}/{max(map(len, sadj))}"
        print(f"{name:8s} {lv / b:12.1f} {ev:12d} {ev / (b * n):6.2f} {stc:10d} {op:10d}"
              f" {r['need']:10d} {r['open_g']:10d} {r['need_g']:10d} {crit:>17s} {per:>11s} {deg:>10s}", flush=True)


if __name__ == "__main__":
    main(sys.argv)
