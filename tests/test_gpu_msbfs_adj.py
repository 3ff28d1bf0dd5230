"""The multi-source BFS's adjacency skip (spf_msbfs_kernel's kMsSkipAdj,
ORH_MS_ADJ; on by default in cluster order): a slice runs a level only if a
slice holding a neighbour of its nodes, or itself, gained a bit the level
before. Every dist entry and every first-hop mask word of the checked rows
exact against the faithful oracle's runSpf tables, with the helpers and
graphs of test_gpu_msbfs_cluster.py.

Unless a case says otherwise it runs under ORH_MS_ORDER=cluster with
ORH_BFS_NH_MAX=0 and ORH_MS_BLOCK=64 (one wave), and `ms_adj == 1` is
asserted.

  grid 20x20    all sources at one wave (J = 8) and at two (marks cross
                waves); once more with ORH_MS_ADJ=0: the same rows, ms_adj 0
  components    an isolated node, a path, a 7x10 mesh with an overloaded node
                and a drained link: slices that are never todo (INF rows)
  wheel         the hub's continuation records: overflow neighbours must be
                in the adjacency
  ring          N = 64 * 32 - 37 (J = 32), K in {4, 8}, 96 scattered sources:
                level-0 marks in arbitrary slices, chords between far slices,
                neighbour-only rows
  ladder        2 x 300 with b295 cut off: levels >= 254 written directly
  restored      a ring loaded with its one chord drained, the chord restored
                through update_adjacency_database: the adjacency covers it
  envelope      rings of 256 slices (the most the bitmasks take: ms_adj 1)
                and of 257 (ms_adj 0), 64 sources, 1,024 threads
  forced        ORH_MS_ADJ=1 under Cuthill-McKee order
  plans         the latency plan (a batch alone on its CU) leaves the mode
                off, ORH_MS_ADJ=1 takes it there too; the same rows
"""
import copy
import random

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import int_topology, ladder
from openr_amd.types import K_TESTING_AREA
from test_gpu_msbfs_cluster import _graph, _sweep, _three_components, grid20, rings  # noqa: F401 (fixtures)
from test_gpu_msbfs_shapes import N_SOURCES, _ms_j, _ring_with_chords
from test_gpu_weighted import _compare_rows

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
MSBFS = 1
INF = 0xFFFFFFFF


@pytest.fixture(autouse=True)
def _adj_plan(monkeypatch):
    for k in ("ORH_MS_LATENCY", "ORH_MS_SKIP", "ORH_MS_DIRECT", "ORH_MS_WIDE", "ORH_HOP_DIST", "ORH_MS_SORT",
              "ORH_MS_ADJ"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("ORH_BFS_NH_MAX", "0")
    monkeypatch.setenv("ORH_MS_BLOCK", "64")
    monkeypatch.setenv("ORH_MS_ORDER", "cluster")


def _adj_sweep(hip, g, adj=1, **kw):
    sw, order, info = _sweep(hip, g, **kw)
    assert info["ms_adj"] == adj, info
    return sw, info


@pytest.mark.parametrize("block", [64, 128])
def test_grid20_all_sources_and_off(hip, grid20, monkeypatch, block):
    """One wave (J = 8) and two (J = 4: a slice's marks are read by the other
    wave); ORH_MS_ADJ=0 gives the same rows without the mode."""
    monkeypatch.setenv("ORH_MS_BLOCK", str(block))
    assert _ms_j(400, block) == (8 if block == 64 else 4)
    sw_on, _ = _adj_sweep(hip, grid20, block=block)
    monkeypatch.setenv("ORH_MS_ADJ", "0")
    sw_off, _ = _adj_sweep(hip, grid20, adj=0, block=block)
    for i in range(len(grid20["names"])):
        d0, m0 = sw_on.fetch(i)
        d1, m1 = sw_off.fetch(i)
        assert np.array_equal(d0, d1) and np.array_equal(m0, m1), grid20["names"][i]


def test_three_components(hip, oracle):
    """Slices of another component are never todo: INF rows, no hops."""
    g = _graph(hip, oracle, _three_components())
    far = g["dist"] == INF
    assert far.any(axis=1).all() and not g["nh"][far].any()
    sw, _ = _adj_sweep(hip, g)
    d, m = sw.fetch(g["names"].index("3"))
    at = [g["order"].index(str(v)) for v in range(6, 76)]
    assert (d[at] == INF).all() and not m.reshape(len(d), -1)[at].any()


def test_wheel48_overflow_neighbours(hip, oracle):
    """Hub 0, a rim 1..48, two pendant nodes a rim node (N = 145, three
    slices): most of the hub's neighbours sit behind its continuation record,
    and they must count for the adjacency."""
    m = 48
    adj = {0: list(range(1, m + 1))}
    for i in range(1, m + 1):
        adj[i] = [0, i % m + 1, (i - 2) % m + 1, m + 2 * i - 1, m + 2 * i]
        adj[m + 2 * i - 1] = [i]
        adj[m + 2 * i] = [i]
    g = _graph(hip, oracle, int_topology(adj))
    assert len(g["order"]) == 145
    _adj_sweep(hip, g)


@pytest.mark.parametrize("k", [4, 8])
def test_ring_with_chords_j32(hip, rings, k):
    """96 scattered sources: level 0 marks arbitrary slices, chords join far
    slices, neighbour-only rows ride along."""
    n = 64 * 32 - 37
    assert _ms_j(n, 64) == 32
    _, info = _adj_sweep(hip, rings(n, k))
    assert info["rows"] > N_SOURCES, info


def test_ladder_deep_levels(hip, oracle):
    """2 x 300 ladder, b295 cut off: levels >= 254 are written during the
    search (kLvlDirect) by slices the skip lets run."""
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
    _adj_sweep(hip, g)


def _set_chord(dbs, a, b, drained):
    out = []
    for x, y in ((a, b), (b, a)):
        db = next(d for d in dbs if d.thisNodeName == str(x))
        for ad in db.adjacencies:
            if ad.otherNodeName == str(y):
                ad.isOverloaded = drained
        out.append(db)
    return out


def test_restored_link_is_in_the_adjacency(hip, oracle):
    """A 400-node ring whose one chord 105 - 305 is drained at the load: the
    chord alone joins its ends' slices (the cluster order grows through most
    other chords and puts both ends into one slice). Restored through
    update_adjacency_database, it brings the ends from 200 hops to 1, and the
    sweep after it must find that: the adjacency is built from down records
    too."""
    from openr_amd import _openr_host
    n, ca, cb = 400, 105, 305
    adj = {v: [(v + 1) % n, (v - 1) % n] for v in range(n)}
    adj[ca].append(cb)
    adj[cb].append(ca)
    dbs = int_topology(adj)
    _set_chord(dbs, ca, cb, True)
    names = [str(v) for v in range(n)]
    als_h, _ = load_topology(hip, dbs, [])
    als_o, _ = load_topology(oracle, dbs, [])
    ls = als_h[A]._impl
    kind, order = ls.ms_order()
    assert kind == "cluster"
    at = {v: i for i, v in enumerate(order)}
    sa, sb = at[str(ca)] // 64, at[str(cb)] // 64
    ring = [[(v + 1) % n, (v - 1) % n] for v in range(n)]
    without, _ = _openr_host.ms_slice_adjacency(ring, [int(v) for v in order])
    assert sa != sb and sb not in without[sa] and sa not in without[sb]  # joined by the chord alone

    def tables():
        return als_o[A]._impl.spf_tables(names, ls.node_names(), [ls.neighbors(s) for s in names], 16)

    def sweep():
        sw = ls.sweep(names, True)
        sw.run()
        sw.sync()
        info = sw.info()
        assert info["variant"] == MSBFS and info["ms_adj"] == 1 and info["ms_skip"] == 0, info
        return sw

    dist_d, nh_d = tables()
    _compare_rows(sweep(), names, list(range(n)), dist_d, nh_d, "oracle, chord drained")
    for db in _set_chord(copy.deepcopy(dbs), ca, cb, False):
        als_h[A].update_adjacency_database(db)
        als_o[A].update_adjacency_database(db)
    dist_r, nh_r = tables()
    col = ls.node_names().index(str(cb))
    assert dist_d[ca][col] == 200 * dist_r[ca][col]
    _compare_rows(sweep(), names, list(range(n)), dist_r, nh_r, "oracle, chord restored")


@pytest.mark.parametrize("n,adj_on,bits", [(64 * 256 - 37, 1, 32), (64 * 256 + 27, 0, 16)])
def test_envelope_edge(hip, oracle, monkeypatch, n, adj_on, bits):
    """256 slices are the most the kernel's bitmasks take (8 words); a graph of
    257 sweeps without the mode. 64 sources at 1,024 threads (J = 16 and 20;
    one wave would need J > 32)."""
    monkeypatch.setenv("ORH_MS_BLOCK", "1024")
    assert (n + 63) // 64 == 257 - adj_on
    adj, hub = _ring_with_chords(n, 4)
    dbs = int_topology(adj)
    rng = random.Random(n)
    srcs = [str(hub)] + [str(v) for v in rng.sample([v for v in range(n) if v != hub], 63)]
    als_h, _ = load_topology(hip, dbs, [])
    als_o, _ = load_topology(oracle, dbs, [])
    ls = als_h[A]._impl
    assert ls.ms_order()[0] == "cluster"
    dist_o, nh_o = als_o[A]._impl.spf_tables(srcs, ls.node_names(), [ls.neighbors(s) for s in srcs], 16)
    assert not (dist_o == INF).any()
    sw = ls.sweep(srcs, True)
    sw.run()
    sw.sync()
    info = sw.info()
    assert info["variant"] == MSBFS and info["mask_bits"] == bits and info["ms_skip"] == 0, info
    assert info["ms_adj"] == adj_on, info
    _compare_rows(sw, srcs, list(range(len(srcs))), dist_o, nh_o, "oracle")


def test_forced_under_cuthill_mckee(hip, grid20, monkeypatch):
    """ORH_MS_ADJ=1 takes the mode under any order; Cuthill-McKee alone
    leaves it off."""
    monkeypatch.setenv("ORH_MS_ORDER", "cm")
    _adj_sweep(hip, grid20, adj=0, kind="cm")
    monkeypatch.setenv("ORH_MS_ADJ", "1")
    _adj_sweep(hip, grid20, kind="cm")


@pytest.mark.parametrize("forced", [0, 1])
def test_latency_plan_leaves_it_off(hip, grid20, monkeypatch, forced):
    """The planner's own shape for 400 sources (13 batches, a CU each, 1,024
    threads): the mode measured slower there, so it is off unless
    ORH_MS_ADJ=1 asks for it."""
    monkeypatch.delenv("ORH_MS_BLOCK")
    if forced:
        monkeypatch.setenv("ORH_MS_ADJ", "1")
    _adj_sweep(hip, grid20, adj=forced, block=1024)
