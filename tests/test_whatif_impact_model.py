"""tests/impact_model.py, the reference of the what-if impact records, pinned on
two hand-worked cases (no GPU). The rows are written out by hand and also
re-derived by a small breadth-first search, so a slip in either shows."""
from collections import deque

import numpy as np

from impact_model import FIELDS, INF, NO_NODE, impact_classes, impact_record, node_counts


def _bfs_row(adj, src, cut=None):
    """Unit-metric SPF row: (dist, first-hop mask), bit b = the b-th smallest
    neighbour of src; ``cut`` is an undirected link (a, b) to ignore."""
    n = len(adj)
    nbrs = sorted(adj[src])
    dist = np.full(n, INF, np.uint32)
    nh = np.zeros(n, np.uint32)
    dist[src] = 0
    q = deque([src])
    while q:
        u = q.popleft()
        for v in sorted(adj[u]):
            if cut and {u, v} == set(cut):
                continue
            if dist[v] == INF:
                dist[v] = dist[u] + 1
                q.append(v)
            if dist[v] == dist[u] + 1:
                nh[v] |= (1 << nbrs.index(v)) if u == src else nh[u]
    return dist, nh


def _ring(n):
    return {v: [(v - 1) % n, (v + 1) % n] for v in range(n)}


def _grid(k):
    adj = {v: [] for v in range(k * k)}
    for r in range(k):
        for c in range(k):
            v = r * k + c
            if c + 1 < k:
                adj[v].append(v + 1)
                adj[v + 1].append(v)
            if r + 1 < k:
                adj[v].append(v + k)
                adj[v + k].append(v)
    return adj


def test_ring_of_8_link_0_1_cut():
    """Source 0, first hops 1 (bit 0) and 7 (bit 1). Without 0-1 everything
    goes round through 7: 1, 2, 3 go 1 -> 7, 2 -> 6, 3 -> 5; node 4 keeps
    distance 4 and loses the hop through 1."""
    base = (np.array([0, 1, 2, 3, 4, 3, 2, 1], np.uint32), np.array([0, 1, 1, 1, 3, 2, 2, 2], np.uint32))
    req = (np.array([0, 7, 6, 5, 4, 3, 2, 1], np.uint32), np.array([0, 2, 2, 2, 2, 2, 2, 2], np.uint32))
    for hand, derived in ((base, _bfs_row(_ring(8), 0)), (req, _bfs_row(_ring(8), 0, (0, 1)))):
        assert np.array_equal(hand[0], derived[0]) and np.array_equal(hand[1], derived[1])
    rec = impact_record(*base, *req, src=0)
    assert rec == dict(lost=0, farther=3, rehomed=1, narrowed=1, max_stretch=6, worst_node=1, sum_stretch=12,
                       lost_weight=0, moved_weight=0)
    assert tuple(rec) == FIELDS
    w = np.array([100, 1, 2, 4, 8, 16, 32, 64], np.uint32)
    rec = impact_record(*base, *req, src=0, weight=w)
    assert rec["lost_weight"] == 0 and rec["moved_weight"] == 1 + 2 + 4 + 8


def test_grid_3x3_link_0_1_cut_ties_to_the_smallest_id():
    """Row-major ids, source 0, first hops 1 (bit 0) and 3 (bit 1). Without
    0-1 every node is reached through 3 only: 1 and 2 both stretch by 2 (the
    tie: worst_node = 1); 4, 5, 7, 8 keep their distance and drop hop 1."""
    base = (np.array([0, 1, 2, 1, 2, 3, 2, 3, 4], np.uint32), np.array([0, 1, 1, 2, 3, 3, 2, 3, 3], np.uint32))
    req = (np.array([0, 3, 4, 1, 2, 3, 2, 3, 4], np.uint32), np.array([0, 2, 2, 2, 2, 2, 2, 2, 2], np.uint32))
    for hand, derived in ((base, _bfs_row(_grid(3), 0)), (req, _bfs_row(_grid(3), 0, (0, 1)))):
        assert np.array_equal(hand[0], derived[0]) and np.array_equal(hand[1], derived[1])
    rec = impact_record(*base, *req, src=0)
    assert rec == dict(lost=0, farther=2, rehomed=4, narrowed=4, max_stretch=2, worst_node=1, sum_stretch=4,
                       lost_weight=0, moved_weight=0)


def test_lost_nodes_base_unreached_nodes_and_sums_past_32_bits():
    """Node 3 is unreached in both rows (no class), 4 and 5 are lost, the
    source's own entry never counts; the weights sum in 64 bits."""
    base = (np.array([0, 2, 3, INF, 5, 6], np.uint32), np.array([0, 1, 1, 0, 1, 1], np.uint32))
    req = (np.array([0, 2, 3, INF, INF, INF], np.uint32), np.array([7, 1, 1, 0, 0, 0], np.uint32))
    w = np.array([9, 9, 9, 9, 0xFFFFFFFF, 0x80000000], np.uint32)
    rec = impact_record(*base, *req, src=0, weight=w)
    assert rec == dict(lost=2, farther=0, rehomed=0, narrowed=0, max_stretch=0, worst_node=NO_NODE,
                       sum_stretch=0, lost_weight=0x17FFFFFFF, moved_weight=0x17FFFFFFF)
    same = impact_record(*base, *base, src=0, weight=w)
    assert all(same[f] == 0 for f in FIELDS if f != "worst_node") and same["worst_node"] == NO_NODE
    lost, moved = node_counts([impact_classes(*base, *req, src=0), impact_classes(*base, *base, src=0)])
    assert lost.tolist() == [0, 0, 0, 0, 1, 1] and moved.tolist() == [0, 0, 0, 0, 1, 1]
