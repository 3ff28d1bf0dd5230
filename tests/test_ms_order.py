"""The node orders of the multi-source layouts (csrc/host/ms_order.h) without
a device: the C++ functions through `_openr_host.ms_orders` against their
restatement in tools/ms_order_model.py, the properties the cluster order
promises, and the model's figures on the 40x40 grid (Cuthill-McKee's are the
recorded ones: 1,272,070 events, 48,540 store instructions, 68,348 open
slice-levels)."""
import importlib.util
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_model():
    spec = importlib.util.spec_from_file_location("ms_order_model", os.path.join(ROOT, "tools", "ms_order_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


model = _load_model()


@pytest.fixture(scope="module")
def host():
    from openr_amd import _openr_host
    return _openr_host


def _three_components():
    """An isolated node, a 5-node path and a 70-node mesh (7 x 10 grid)."""
    adj = {0: []}
    for i in range(1, 6):
        adj[i] = [j for j in (i - 1, i + 1) if 1 <= j <= 5]
    for r in range(7):
        for c in range(10):
            adj[6 + r * 10 + c] = sorted(6 + rr * 10 + cc for rr, cc in ((r, c + 1), (r, c - 1), (r - 1, c), (r + 1, c))
                                         if 0 <= rr < 7 and 0 <= cc < 10)
    return [adj[v] for v in range(76)]


def _wheel(spokes):
    adj = [list(range(1, spokes + 1))]
    for i in range(1, spokes + 1):
        adj.append(sorted({0, 1 + i % spokes, 1 + (i - 2) % spokes}))
    return adj


def _random_graph(n, seed):
    rng = random.Random(seed)
    adj = [set() for _ in range(n)]
    for _ in range(2 * n):
        a, b = rng.randrange(n), rng.randrange(n)
        if a != b:
            adj[a].add(b)
            adj[b].add(a)
    return [sorted(a) for a in adj]


GRAPHS = {
    "grid20": lambda: model.grid(20),
    "grid40": lambda: model.grid(40),
    "ring219": lambda: model.ring_with_chords(219, 4),
    "ring2011_k8": lambda: model.ring_with_chords(2011, 8),
    "components": _three_components,
    "wheel48": lambda: _wheel(48),
    "random500": lambda: _random_graph(500, 5),  # several components, isolated nodes
    "empty": lambda: [],
    "single": lambda: [[]],
}


def _components(adj):
    comp = [-1] * len(adj)
    for s in range(len(adj)):
        if comp[s] >= 0:
            continue
        comp[s] = s
        todo = [s]
        while todo:
            v = todo.pop()
            for u in adj[v]:
                if comp[u] < 0:
                    comp[u] = s
                    todo.append(u)
    return comp


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_orders_match_the_model_and_hold_their_properties(host, name):
    adj = GRAPHS[name]()
    n = len(adj)
    cm, depth, cluster = host.ms_orders(adj)
    cm_py, depth_py = model.cm_order(adj)
    assert list(cm) == cm_py and depth == depth_py
    assert list(cluster) == model.cluster_order(adj, cm_py)
    assert sorted(cluster) == list(range(n))  # a bijection onto dense ids
    # components take contiguous id ranges: a run of 64 mixes components only
    # where one ends inside it
    comp = _components(adj)
    seen = []
    for v in cluster:
        if not seen or seen[-1] != comp[v]:
            seen.append(comp[v])
    assert len(seen) == len(set(seen))
    # a run is grown by BFS: a node with no neighbour earlier in its run
    # starts a piece (the run's first seed, or a pocket's). On the grids fewer
    # than one run in two holds a second piece
    if name.startswith("grid"):
        pieces = 0
        for r0 in range(0, n, 64):
            run = cluster[r0:r0 + 64]
            pieces += sum(1 for i, v in enumerate(run) if not set(run[:i]).intersection(adj[v]))
        runs = (n + 63) // 64
        print(name, "runs", runs, "pieces", pieces)
        assert pieces <= runs + runs // 2, pieces


def test_grid_depth_and_clos_depth(host):
    """What the default selection reads: Cuthill-McKee's BFS depth."""
    _, depth, _ = host.ms_orders(model.grid(100))
    assert depth == 198
    # a 3-tier Clos: 8 spines, 16 fabric switches, 64 racks
    adj = [[] for _ in range(88)]
    for f in range(16):
        for s in range(8):
            adj[8 + f].append(s)
            adj[s].append(8 + f)
    for r in range(64):
        for f in range(4):
            a, b = 24 + r, 8 + (r // 16) * 4 + f
            adj[a].append(b)
            adj[b].append(a)
    _, depth, _ = host.ms_orders([sorted(a) for a in adj])
    assert depth <= 6


def test_model_figures_40x40():
    adj = model.grid(40)
    cm, _ = model.cm_order(adj)
    _, _, ev, st, op = model.model(adj, cm)
    assert (ev, st, op) == (1272070, 48540, 68348)
    _, _, ev_c, st_c, op_c = model.model(adj, model.cluster_order(adj, cm))
    print("cluster 40x40: events", ev_c, "stores", st_c, "open", op_c)
    assert st_c <= 0.8 * st and op_c <= 0.85 * op
    assert ev_c < ev
