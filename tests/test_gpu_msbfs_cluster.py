"""The multi-source BFS in the cluster node order (ms_cluster_order,
csrc/host/ms_order.h; ORH_MS_ORDER=cluster, and by default on deep graphs):
every dist entry and every first-hop mask word of the checked rows exact
against the faithful oracle's runSpf tables (LinkState.cpp:808-882).

Unless a case says otherwise it runs under ORH_MS_ORDER=cluster with
ORH_BFS_NH_MAX=0 (no fused per-source BFS) and ORH_MS_BLOCK=64 (one wave, J a
function of N alone).

  grid 20x20    N = 400: six full clusters and a 16-node remainder; all
                sources; once more at 128 threads (two waves)
  ring          N = 64 J - 37, J in {4, 32} x K in {4, 8}, 96 sources
                (neighbour-only rows); J = 32: the end of the log's node
                field, the large assembly LDS
  components    an isolated node, a 5-node path, a 7x10 mesh with an
                overloaded node and a drained link: INF rows without hops,
                components in contiguous ids
  ladder        2 x 300 with an isolated node: levels >= 254 written through
                host_of (kLvlDirect)
  wheel         a hub of 48 rim nodes with two pendant nodes each: continuation
                records, a cluster that ends in the middle of a neighbour list
  skip          ORH_MS_SKIP=1 and ORH_MS_LATENCY=2 on the 20x20 grid: the
                interval skip with the cluster order's bandwidth
  the order     a bijection onto dense ids; on the 40x40 grid its modelled
                store instructions <= 0.8x and open slice-levels <= 0.85x
                Cuthill-McKee's (tools/ms_order_model.py; CPU figures 0.63x /
                0.72x)
  default       the 100x100 grid takes the cluster order (20 rows in full:
                corners, the centre, what-if variant 7's drained link); the
                400-node Clos keeps Cuthill-McKee; ORH_MS_ORDER=cm on the
                20x20 grid gives the default's rows
"""
import importlib.util
import os
import random

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid, int_topology, ladder
from openr_amd.types import K_TESTING_AREA
from openr_amd.workloads import c3_weighted_fabric
from test_gpu_hop_dist import _oracle_tables
from test_gpu_msbfs_shapes import N_SOURCES, _ell_k, _ms_j, _ring_with_chords
from test_gpu_weighted import _compare_rows

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
MSBFS = 1
INF = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_model():
    spec = importlib.util.spec_from_file_location("ms_order_model", os.path.join(ROOT, "tools", "ms_order_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(autouse=True)
def _cluster_plan(monkeypatch):
    for k in ("ORH_MS_LATENCY", "ORH_MS_SKIP", "ORH_MS_DIRECT", "ORH_MS_WIDE", "ORH_HOP_DIST", "ORH_MS_SORT"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ORH_BFS_NH_MAX", "0")
    monkeypatch.setenv("ORH_MS_BLOCK", "64")
    monkeypatch.setenv("ORH_MS_ORDER", "cluster")


def _graph(hip, oracle, dbs):
    """The oracle's tables of every node as a source (rows in sorted-name
    order), computed once, read-only, shared by the cases that run the graph."""
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    dist_o, nh_o = _oracle_tables(oracle, ls, dbs)
    return {"dbs": dbs, "names": sorted(db.thisNodeName for db in dbs), "order": ls.node_names(), "dist": dist_o,
            "nh": nh_o}


def _sweep(hip, g, kind="cluster", block=64, skip=0, srcs=None, rows=None):
    """One sweep on a fresh device mirror (the layout reads the environment at
    its load); the order the graph took, the kernel shape, all rows."""
    als_h, _ = load_topology(hip, g["dbs"], [])
    ls = als_h[A]._impl
    assert ls.node_names() == g["order"]
    got_kind, order = ls.ms_order()
    assert got_kind == kind
    assert sorted(order) == sorted(g["order"])  # a bijection: every node once
    names = g["names"] if srcs is None else srcs
    sw = ls.sweep(names, True)
    sw.run()
    sw.sync()
    info = sw.info()
    assert info["variant"] == MSBFS and info["mask_bits"] == 32 and info["batch_sources"] == 32, info
    assert info["ms_direct"] == 0 and info["ms_skip"] == skip, info
    if block:
        assert info["ms_threads"] == block, info
    rows = list(range(len(names))) if rows is None else rows
    at = [g["names"].index(names[i]) for i in rows]
    _compare_rows(sw, names, rows, g["dist"][at], g["nh"][at], "oracle")
    return sw, order, info


@pytest.fixture(scope="module")
def grid20(hip, oracle):
    return _graph(hip, oracle, bench_grid(20)[0])


@pytest.mark.parametrize("block", [64, 128])
def test_grid20_all_sources(hip, grid20, monkeypatch, block):
    """N = 400: six full clusters and a remainder of 16; at 128 threads the
    log assembly's per-wave loop runs twice."""
    monkeypatch.setenv("ORH_MS_BLOCK", str(block))
    assert _ms_j(400, block) == (8 if block == 64 else 4)
    _, order, _ = _sweep(hip, grid20, block=block)
    assert len(order) == 400 == 6 * 64 + 16
    # the first cluster is one BFS ball grown from Cuthill-McKee's root, a
    # corner: 64 nodes within 10 hops of it (1 + 2 + ... + 11 = 66 >= 64)
    r0, c0 = divmod(int(order[0]), 20)
    assert (r0, c0) in ((0, 0), (0, 19), (19, 0), (19, 19))
    assert all(abs(int(v) // 20 - r0) + abs(int(v) % 20 - c0) <= 10 for v in order[:64])


@pytest.fixture(scope="module")
def rings(hip, oracle):
    memo = {}

    def get(n, k):
        if (n, k) not in memo:
            adj, hub = _ring_with_chords(n, k)
            dbs = int_topology(adj)
            assert _ell_k(dbs) == k and len(set(adj[hub])) >= 12  # a continuation record at either K
            rng = random.Random(n + k)
            srcs = [str(hub)] + [str(v) for v in rng.sample([v for v in range(n) if v != hub], N_SOURCES - 1)]
            als_h, _ = load_topology(hip, dbs, [])
            als_o, _ = load_topology(oracle, dbs, [])
            ls = als_h[A]._impl
            dist_o, nh_o = als_o[A]._impl.spf_tables(srcs, ls.node_names(), [ls.neighbors(s) for s in srcs], 16)
            dist_o.setflags(write=False)
            nh_o.setflags(write=False)
            assert int(dist_o.max()) > 32 and not (dist_o == INF).any()
            memo[(n, k)] = {"dbs": dbs, "names": srcs, "order": ls.node_names(), "dist": dist_o, "nh": nh_o}
        return memo[(n, k)]

    return get


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("j", [4, 32])
def test_ring_with_chords(hip, rings, j, k):
    """spf_msbfs_kernel<k, u32, j, false> in cluster order; 96 sources leave
    neighbour-only rows."""
    n = 64 * j - 37
    assert _ms_j(n, 64) == j
    _, _, info = _sweep(hip, rings(n, k))
    assert info["rows"] > N_SOURCES, info


def _three_components():
    """Node 0 alone, a path 1..5 and a 7 x 10 mesh 6..75; mesh node 40
    overloaded, mesh link 33-34 drained."""
    adj = {0: []}
    for i in range(1, 6):
        adj[i] = [j for j in (i - 1, i + 1) if 1 <= j <= 5]
    for r in range(7):
        for c in range(10):
            adj[6 + r * 10 + c] = [6 + rr * 10 + cc for rr, cc in ((r, c + 1), (r, c - 1), (r - 1, c), (r + 1, c))
                                   if 0 <= rr < 7 and 0 <= cc < 10]
    dbs = int_topology(adj)
    dbs[40].isOverloaded = True
    for a, b in ((33, 34), (34, 33)):
        for ad in dbs[a].adjacencies:
            if ad.otherNodeName == str(b):
                ad.isOverloaded = True
    return dbs


def test_three_components(hip, oracle):
    """Unreachable entries are INF without hops, and no run of 64 ids mixes
    components except where one ends inside it."""
    g = _graph(hip, oracle, _three_components())
    assert len(g["order"]) == 76
    comp = {str(v): (0 if v == 0 else 1 if v <= 5 else 2) for v in range(76)}
    row0 = g["dist"][g["names"].index("0")]
    assert (row0 == INF).sum() == 75  # the isolated node reaches itself alone
    far = g["dist"] == INF
    assert far.any(axis=1).all() and not g["nh"][far].any()
    sw, order, _ = _sweep(hip, g)
    seen = []
    for v in order:
        if not seen or seen[-1] != comp[v]:
            seen.append(comp[v])
    assert len(seen) == 3, seen  # each component one contiguous id range
    d, m = sw.fetch(g["names"].index("3"))
    at = [g["order"].index(str(v)) for v in range(6, 76)]
    assert (d[at] == INF).all() and not m.reshape(len(d), -1)[at].any()


def test_ladder_deep_levels_with_isolated_node(hip, oracle):
    """2 x 300 ladder, b295 cut off: levels >= 254 are written during the
    search through host_of (kLvlDirect), next to 255 bytes."""
    dbs = ladder(300, 1)[0]
    by_name = {db.thisNodeName: db for db in dbs}
    for adj in by_name["b295"].adjacencies:
        adj.isOverloaded = True
        for back in by_name[adj.otherNodeName].adjacencies:
            if back.otherNodeName == "b295":
                back.isOverloaded = True
    g = _graph(hip, oracle, dbs)
    finite = np.where(g["dist"] == INF, 0, g["dist"])
    assert int(finite.max()) == 301 and (g["dist"] == INF).any(axis=1).all()
    assert _ms_j(600, 64) == 12
    _sweep(hip, g)


def test_wheel48_continuation_records(hip, oracle):
    """Hub 0, a rim 1..48 and two pendant nodes on every rim node (N = 145):
    the hub's ELL row ends in a continuation record, and the first cluster
    fills up in the middle of a rim node's neighbour list. (The seed is a
    pendant node; its rim node, the hub and the rim bring the cluster to 51
    nodes, and 13 pendants in pairs end inside a pair.)"""
    m = 48
    adj = {0: list(range(1, m + 1))}
    for i in range(1, m + 1):
        adj[i] = [0, i % m + 1, (i - 2) % m + 1, m + 2 * i - 1, m + 2 * i]
        adj[m + 2 * i - 1] = [i]
        adj[m + 2 * i] = [i]
    g = _graph(hip, oracle, int_topology(adj))
    assert len(g["order"]) == 145
    _, order, _ = _sweep(hip, g)
    run = order[:64]
    assert "0" in run
    # the node that was being expanded when the run filled up is the earliest
    # of the run next to its last node; it keeps a neighbour for a later run
    nbrs = {str(v): {str(u) for u in adj[v]} for v in adj}
    expanding = next(v for v in run if run[-1] in nbrs[v])
    assert nbrs[expanding] - set(run), (expanding, run)


@pytest.mark.parametrize("knob", ["ORH_MS_SKIP=1", "ORH_MS_LATENCY=2"])
def test_grid20_interval_skip(hip, grid20, monkeypatch, knob):
    """spf_msbfs_kernel<..., true> with the cluster order's bandwidth;
    ORH_MS_LATENCY=2 needs the planner (no ORH_MS_BLOCK): 13 batches, each on
    a CU of its own, 1,024 threads."""
    name, val = knob.split("=")
    monkeypatch.setenv(name, val)
    if name == "ORH_MS_LATENCY":
        monkeypatch.delenv("ORH_MS_BLOCK")
        _sweep(hip, grid20, block=1024, skip=1)
    else:
        _sweep(hip, grid20, skip=1)


def test_order_model_40x40(hip, monkeypatch):
    """The order the library built for the 40x40 grid, in the model: store
    instructions <= 0.8x and open slice-levels <= 0.85x Cuthill-McKee's."""
    model = _load_model()
    dbs, _ = bench_grid(40)
    orders = {}
    for kind in ("cm", "cluster"):
        monkeypatch.setenv("ORH_MS_ORDER", kind)
        als_h, _ = load_topology(hip, dbs, [])
        got, order = als_h[A]._impl.ms_order()
        assert got == kind
        orders[kind] = [int(v) for v in order]
        assert sorted(orders[kind]) == list(range(1600))  # a bijection, dense ids
    adj = model.grid(40)
    _, _, ev_cm, st_cm, op_cm = model.model(adj, orders["cm"])
    _, _, ev_cl, st_cl, op_cl = model.model(adj, orders["cluster"])
    print("40x40 cm", ev_cm, st_cm, op_cm, "cluster", ev_cl, st_cl, op_cl)
    assert st_cl <= 0.8 * st_cm, (st_cl, st_cm)
    assert op_cl <= 0.85 * op_cm, (op_cl, op_cm)


def test_default_grid100_takes_cluster(hip, oracle, monkeypatch):
    """The benched grid under the default selection and the default planner:
    cluster order, 20 rows in full - the corners, the centre and seeded ones -
    on what-if variant 7 (bench.py: link 7 drained)."""
    from bench import drain_what_if_link
    monkeypatch.delenv("ORH_MS_ORDER")
    monkeypatch.delenv("ORH_MS_BLOCK")
    monkeypatch.delenv("ORH_BFS_NH_MAX")
    n = 100
    dbs, _ = bench_grid(n)
    assert drain_what_if_link(dbs, n, 7)
    als_h, _ = load_topology(hip, dbs, [])
    als_o, _ = load_topology(oracle, dbs, [])
    ls = als_h[A]._impl
    kind, order = ls.ms_order()
    assert kind == "cluster" and sorted(order, key=int) == [str(v) for v in range(n * n)]
    names = [str(v) for v in range(n * n)]
    sw = ls.sweep(names, True)
    sw.run()
    sw.sync()
    info = sw.info()
    assert info["variant"] == MSBFS and info["mask_bits"] == 32 and info["batch_sources"] == 32, info
    assert info["ms_direct"] == 0 and info["ms_skip"] == 0 and info["hop_nodes"] == 8, info
    rng = random.Random(100)
    fixed = [0, n - 1, n * (n - 1), n * n - 1, n * (n // 2) + n // 2]
    check = fixed + rng.sample([v for v in range(n * n) if v not in fixed], 15)
    srcs = [names[i] for i in check]
    dist_o, nh_o = als_o[A]._impl.spf_tables(srcs, ls.node_names(), [ls.neighbors(s) for s in srcs], 16)
    _compare_rows(sw, names, check, dist_o, nh_o, "oracle")


def test_default_clos_keeps_cm(hip, monkeypatch):
    """The 400-node Clos of test_gpu_spf_plan_table.py (depth <= 6)."""
    monkeypatch.delenv("ORH_MS_ORDER")
    dbs = c3_weighted_fabric(400, 4, 7)[0]
    als_h, _ = load_topology(hip, dbs, [])
    kind, order = als_h[A]._impl.ms_order()
    assert kind == "cm" and len(order) == len(set(order)) == len(als_h[A]._impl.node_names())


def test_grid20_cm_equals_default(hip, grid20, monkeypatch):
    """ORH_MS_ORDER=cm keeps meaning Cuthill-McKee; its rows are the
    default's (the 20x20 grid is 38 levels deep: cluster by default)."""
    monkeypatch.setenv("ORH_MS_ORDER", "cm")
    sw_cm, _, _ = _sweep(hip, grid20, kind="cm")
    monkeypatch.delenv("ORH_MS_ORDER")
    sw_def, _, _ = _sweep(hip, grid20, kind="cluster")
    for i in range(len(grid20["names"])):
        d0, m0 = sw_cm.fetch(i)
        d1, m1 = sw_def.fetch(i)
        assert np.array_equal(d0, d1) and np.array_equal(m0, m1), grid20["names"][i]
