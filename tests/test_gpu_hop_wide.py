"""first_hop_lvl_kernel<8> (and <16>) with HopArgs::write_dist at the edges of
its tiles, stores and level encodings, and neighbour-only rows with deep
levels on every first-hop width: every row - dist and every first-hop mask
word - exact against the faithful oracle's runSpf tables
(LinkState.cpp:808-882).

launch_first_hop takes 8 nodes per thread only when ceil(N / 4096) * n_out >=
8192. Sources may repeat in a sweep (stage_request maps a neighbour to the row
of its first occurrence), so a small graph swept k times over reaches that
with oracle tables for its unique sources only; every row, duplicates
included, is compared. ORH_BFS_NH_MAX=0 (read per run) keeps the sweeps on the
MS-BFS plan.

  graph (N)            rows                  what the wide kernel meets
  13x13 + defects 169  all x 49 = 8,281      N % 8 == 1: the tail group, rows
                                             off a 16-byte base, per-element
                                             nh and dist stores, 255 bytes, an
                                             overloaded first hop, an isolated
                                             source
  wheel 81             all x 102 = 8,262     two mask words, ranks 8..39,
                                             block runs of 16 per XCD with an
                                             unremapped tail of 70
  ladder 2x300 600     all x 14 = 8,400      kLvlDirect entries, both orders
  ladder 2x300 600     a* x 28 = 8,400       deep levels of the neighbour-only
                       (+ 300 b* rows)       b* rows read back from scratch
  ladder 2x300 600     a* once = 300         the same on the 4-node kernel
  47x47 + defects 2209 all x 4 = 8,836       N % 4 == 1, one workgroup walking
                                             2 tiles, the second of 161 nodes
  65x65 4225           0..4159 once          hop_split == 2 over 3 tiles (phase
                                             0 walks tiles 0 and 2), the last
                                             grid row neighbour-only

The defects are those of test_gpu_hop_dist's 12x12 case: node 40 overloaded,
link 66-67 drained, node 100 isolated by draining its links.
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid, int_topology, ladder
from openr_amd.types import K_TESTING_AREA
from test_gpu_hop_dist import _oracle_tables, _wheel
from test_gpu_weighted import _compare_rows

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
MSBFS = 1
INF = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS = ["cm", "host"]


@pytest.fixture(autouse=True)
def _ms_bfs_plan(monkeypatch):
    monkeypatch.setenv("ORH_BFS_NH_MAX", "0")
    for k in ("ORH_HOP_DIST", "ORH_MS_ORDER", "ORH_MS_BLOCK", "ORH_MS_LATENCY", "ORH_MS_SKIP",
              "ORH_MS_DIRECT", "ORH_MS_WIDE"):
        monkeypatch.delenv(k, raising=False)


def _ceil(a, b):
    return -(-a // b)


def _hop_shape(n, n_out, wide_nodes=8):
    """launch_first_hop restated: (nodes per thread, tiles, workgroups per
    source) of the level-row first-hop kernel."""
    per = wide_nodes if _ceil(n, 4096) * n_out >= 8192 else 4
    tiles = _ceil(n, 256 * per)
    split = 1
    while split < tiles and split * n_out < 8192:
        split += 1
    return per, tiles, split


def _defect_grid(n):
    """bench_grid(n) with node 40 overloaded, link 66-67 drained and node 100
    isolated (test_gpu_hop_dist.test_grid_12x12_overloaded_drained_isolated)."""
    dbs, _ = bench_grid(n)
    dbs[40].isOverloaded = True
    for x in (66, 100):
        for adj in dbs[x].adjacencies:
            if x == 100 or adj.otherNodeName == "67":
                adj.isOverloaded = True
                for back in dbs[int(adj.otherNodeName)].adjacencies:
                    if back.otherNodeName == str(x):
                        back.isOverloaded = True
    return dbs


def _graph(hip, oracle, dbs):
    """The graph with the oracle's tables of every node as a source (rows in
    sorted-name order), computed once, read-only, shared."""
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    dist_o, nh_o = _oracle_tables(oracle, ls, dbs)
    names = sorted(db.thisNodeName for db in dbs)
    return {"dbs": dbs, "names": names, "order": ls.node_names(), "dist": dist_o, "nh": nh_o,
            "at": {s: k for k, s in enumerate(names)}, "nbrs": {s: ls.neighbors(s) for s in names}}


@pytest.fixture(scope="module")
def grid13(hip, oracle):
    return _graph(hip, oracle, _defect_grid(13))


@pytest.fixture(scope="module")
def wheel(hip, oracle):
    return _graph(hip, oracle, _wheel())


@pytest.fixture(scope="module")
def ladder300(hip, oracle):
    return _graph(hip, oracle, ladder(300, 1)[0])


@pytest.fixture(scope="module")
def grid47(hip, oracle):
    return _graph(hip, oracle, _defect_grid(47))


def _check_rows(fetch, g, srcs):
    """Every row of the sweep over `srcs` (names, repeats allowed) against the
    unique sources' tables."""
    for lo in range(0, len(srcs), 600):
        rows = list(range(lo, min(len(srcs), lo + 600)))
        at = [g["at"][srcs[i]] for i in rows]
        _compare_rows(fetch, srcs, rows, g["dist"][at], g["nh"][at], "oracle")


def _sweep(hip, g, srcs, hop_nodes, hop_dist, ms_direct=0, hop_split=1, extra_rows=0):
    """One sweep on a fresh device mirror; the kernel shape from sweep.info()
    against the arguments and against launch_first_hop restated; all rows."""
    als_h, _ = load_topology(hip, g["dbs"], [])
    ls = als_h[A]._impl
    assert ls.node_names() == g["order"]
    sw = ls.sweep(srcs, True)
    sw.run()
    sw.sync()
    info = sw.info()
    n = len(g["order"])
    assert info["variant"] == MSBFS and info["ms_direct"] == ms_direct, info
    assert info["hop_nodes"] == hop_nodes and info["hop_dist"] == hop_dist, info
    assert info["hop_split"] == hop_split, info
    assert (hop_nodes, hop_split) == _hop_shape(n, len(srcs))[::2]
    assert info["rows"] == len(srcs) + extra_rows, info
    _check_rows(sw, g, srcs)
    return sw, info, ls


def _assert_grid_defects(g):
    """From the CPU tables: every row has an unreached entry, the isolated
    source reaches itself alone, and a source next to the overloaded node has
    it as a first hop towards that node and nothing else."""
    dist, order = g["dist"], g["order"]
    assert np.all((dist == INF).sum(axis=1) >= 1)
    row = dist[g["at"]["100"]]
    assert (row == INF).sum() == len(order) - 1 and row[order.index("100")] == 0
    s = "41"
    assert "40" in g["nbrs"][s]
    bit = g["nbrs"][s].index("40")
    via40 = (g["nh"][g["at"][s]][:, bit // 32] >> (bit % 32)) & 1
    assert via40.sum() == 1 and via40[order.index("40")] == 1


def _xcd_group(g, srcs):
    """stage_request's block order: runs of 16 when the heaviest source has
    more than twice the mean count of neighbour rows."""
    d = [len(g["nbrs"][s]) for s in srcs]
    return 0 if max(d) * len(srcs) <= 2 * sum(d) else 16


def _case_grid13(g):
    srcs = g["names"] * 49
    n = len(g["order"])
    assert n == 169 and n % 8 == 1 and len(srcs) == 8281
    assert _hop_shape(n, len(srcs)) == (8, 1, 1)
    _assert_grid_defects(g)
    return srcs


def test_grid13_defects_tail_and_unaligned_rows(hip, grid13):
    """N = 169, 8,281 rows: the last 8-node group holds one node, odd rows
    start off a 16-byte boundary, and N % 4 != 0 sends every mask store down
    the per-element path."""
    srcs = _case_grid13(grid13)
    sw, _, _ = _sweep(hip, grid13, srcs, 8, 1)
    assert sw.words == 1 and sw.nodes == 169


def _case_wheel(g):
    srcs = g["names"] * 102
    n = len(g["order"])
    assert n == 81 and len(srcs) == 8262
    assert _hop_shape(n, len(srcs)) == (8, 1, 1)
    assert _xcd_group(g, srcs) == 16 and len(srcs) % 128 == 70  # the unremapped tail
    hub = g["nh"][g["at"]["0"]]
    assert hub.shape[1] == 2
    # ranks 0..7 (packed path) and 8..31 (per-node compare) in word 0; the
    # hub's 40 ranks end at bit 7 of word 1, so that word takes the packed path
    assert (hub[:, 0] & 0xFF).any() and (hub[:, 0] >> 8).any()
    assert hub[:, 1].any() and not (hub[:, 1] >> 8).any()
    return srcs


def test_wheel_two_words_high_ranks(hip, wheel):
    """N = 81, 8,262 rows, a hub of 40 neighbours: W == 2, first hops of rank
    8..39 (the per-node compare over both words of the 8-byte level vector),
    and the XCD block order in runs of 16."""
    srcs = _case_wheel(wheel)
    sw, _, _ = _sweep(hip, wheel, srcs, 8, 1)
    assert sw.words == 2


def _wheel48():
    """test_gpu_hop_dist._wheel with 48 spokes: the hub's ranks reach bit 15
    of the second mask word."""
    m = 48
    adj = {0: list(range(1, m + 1))}
    for i in range(1, m + 1):
        nxt, prv = i % m + 1, (i - 2) % m + 1
        adj[i] = [0, nxt, prv, m + i, m + prv]
    for i in range(1, m + 1):
        adj[m + i] = [i, i % m + 1]
    return int_topology(adj)


@pytest.fixture(scope="module")
def wheel48(hip, oracle):
    return _graph(hip, oracle, _wheel48())


def test_wheel48_high_ranks_in_both_words(hip, wheel48):
    """N = 97, 8,245 rows, a hub of 48 neighbours: first hops of rank past 7
    within each of the two mask words (bits >= 8 of both), on N % 8 == 1."""
    g = wheel48
    srcs = g["names"] * 85
    n = len(g["order"])
    assert n == 97 and len(srcs) == 8245 and _hop_shape(n, len(srcs)) == (8, 1, 1)
    assert _xcd_group(g, srcs) == 16
    hub = g["nh"][g["at"]["0"]]
    assert hub.shape[1] == 2 and (hub[:, 0] >> 8).any() and (hub[:, 1] >> 8).any()
    sw, _, _ = _sweep(hip, g, srcs, 8, 1)
    assert sw.words == 2


def _assert_ladder_deep(g, srcs, deepest=300):
    finite = np.where(g["dist"] == INF, 0, g["dist"])
    assert int(finite.max()) == deepest > 254
    deep = finite[[g["at"][s] for s in set(srcs)]].max(axis=1) >= 254
    assert deep.any() and not deep.all()  # rows with and without kLvlDirect entries


@pytest.mark.parametrize("order", ORDERS)
def test_ladder_deep_levels_wide(hip, ladder300, monkeypatch, order):
    """2 x 300 ladder, 8,400 rows: levels >= 254 (kLvlDirect) in the 8-node
    kernel - the direct branch over both words of the level vector, the
    per-element dist store around a 254 byte; rows through ms_finalize_kernel
    + write_dist (cm) and out of the search kernel (host)."""
    monkeypatch.setenv("ORH_MS_ORDER", order)
    g = ladder300
    srcs = g["names"] * 14
    assert len(g["order"]) == 600 and len(srcs) == 8400
    _assert_ladder_deep(g, srcs)
    host = order == "host"
    _sweep(hip, g, srcs, 8, 0 if host else 1, ms_direct=1 if host else 0)


@pytest.fixture(scope="module")
def ladder300_isolated(hip, oracle):
    """The ladder with b295 isolated: from the far end its 255 byte sits in
    one 8-node group with kLvlDirect bytes."""
    dbs = ladder(300, 1)[0]
    by_name = {db.thisNodeName: db for db in dbs}
    for adj in by_name["b295"].adjacencies:
        adj.isOverloaded = True
        for back in by_name[adj.otherNodeName].adjacencies:
            if back.otherNodeName == "b295":
                back.isOverloaded = True
    return _graph(hip, oracle, dbs)


def test_ladder_deep_levels_with_unreached_wide(hip, ladder300_isolated):
    """Deep levels and unreached entries in one row: the direct branch's
    own_dist / dist_at over 254 and 255 bytes side by side."""
    g = ladder300_isolated
    srcs = g["names"] * 14
    _assert_ladder_deep(g, srcs, 301)  # b0 -> b299 around the gap in the b rail
    assert np.all((g["dist"] == INF).sum(axis=1) >= 1)
    row, order = g["dist"][g["at"]["a0"]], g["order"]
    at = order.index("b295")
    group = row[at // 8 * 8:at // 8 * 8 + 8]  # the level rows are in this order
    assert row[at] == INF and ((group >= 254) & (group != INF)).any()
    _sweep(hip, g, srcs, 8, 1)


def _a_rail(g):
    a = [s for s in g["names"] if s.startswith("a")]
    assert len(a) == 300
    # every b* node is some source's neighbour and no source itself
    assert {x for s in a for x in g["nbrs"][s] if x.startswith("b")} == set(g["names"]) - set(a)
    return a


@pytest.mark.parametrize("order", ORDERS)
def test_ladder_neighbour_only_rows_wide(hip, ladder300, monkeypatch, order):
    """Sources = the 300 a* nodes x 28: the b* rows are neighbour-only
    (r >= n_out), so their deep levels go to the scratch rows and the 8-node
    kernel reads them back from there."""
    monkeypatch.setenv("ORH_MS_ORDER", order)
    g = ladder300
    srcs = _a_rail(g) * 28
    assert len(srcs) == 8400
    _assert_ladder_deep(g, srcs)
    host = order == "host"
    _sweep(hip, g, srcs, 8, 0 if host else 1, ms_direct=1 if host else 0, extra_rows=300)


@pytest.mark.parametrize("order", ORDERS)
def test_ladder_neighbour_only_rows_narrow(hip, ladder300, monkeypatch, order):
    """The same a*-only sweep unrepeated, 300 rows: the 4-node kernel."""
    monkeypatch.setenv("ORH_MS_ORDER", order)
    g = ladder300
    srcs = _a_rail(g)
    _assert_ladder_deep(g, srcs)
    host = order == "host"
    _sweep(hip, g, srcs, 4, 0 if host else 1, ms_direct=1 if host else 0, extra_rows=300)


def test_grid47_defects_two_tiles(hip, grid47):
    """N = 2,209, 8,836 rows: N % 4 == 1, and each workgroup walks two tiles,
    the second holding 161 nodes, so threads past it leave at v0 >= N."""
    g = grid47
    srcs = g["names"] * 4
    n = len(g["order"])
    assert n == 2209 and n % 4 == 1 and len(srcs) == 8836
    assert _hop_shape(n, len(srcs)) == (8, 2, 1) and n - 2048 == 161
    _assert_grid_defects(g)
    _sweep(hip, g, srcs, 8, 1)


def test_grid65_split_tiles_neighbour_only_row(hip, oracle):
    """N = 4,225, sources = nodes 0..4159 once: two workgroups per source over
    three tiles (phase 0 walks tiles 0 and 2, the last of 129 nodes), the last
    grid row neighbour-only. Every row against the independent fast checker,
    a seeded 400 - the source block's corners and all of grid row 63 among
    them - against the faithful oracle."""
    n = 65
    dbs, _ = bench_grid(n)
    als_h, _ = load_topology(hip, dbs, [])
    als_o, _ = load_topology(oracle, dbs, [])
    ls = als_h[A]._impl
    order = ls.node_names()
    names = [str(v) for v in range(n * (n - 1))]
    assert len(order) == 4225 and len(names) == 4160
    assert _hop_shape(len(order), len(names)) == (8, 3, 2) and 4225 - 2 * 2048 == 129
    sw = ls.sweep(names, True)
    sw.run()
    sw.sync()
    info = sw.info()
    assert info["variant"] == MSBFS and info["ms_direct"] == 0, info
    assert info["hop_nodes"] == 8 and info["hop_dist"] == 1 and info["hop_split"] == 2, info
    assert info["rows"] == 4225, info
    must = [0, n - 1, n * (n - 2), n * (n - 1) - 1] + list(range(n * (n - 2), n * (n - 1)))
    must = list(dict.fromkeys(must))
    rng = random.Random(65)
    rest = sorted(set(range(len(names))) - set(must))
    check = must + rng.sample(rest, 400 - len(must))
    assert len(check) == 400 and len(set(check)) == 400
    srcs = [names[i] for i in check]
    dist_o, nh_o = als_o[A]._impl.spf_tables(srcs, order, [ls.neighbors(s) for s in srcs], 16)
    _compare_rows(sw, names, check, dist_o, nh_o, "oracle")
    fc = oracle.module.FastChecker(als_o[A]._impl, order)
    ids = {s: i for i, s in enumerate(order)}
    for s in srcs[:8]:  # the checker's mask bits follow the product's neighbour order
        assert [ids[x] for x in ls.neighbors(s)] == list(fc.neighbours(ids[s]))
    dist_f, nh_f = fc.spf_rows([ids[s] for s in srcs], [], 16)
    w = min(nh_f.shape[2], nh_o.shape[2])  # the two references agree where both speak
    assert np.array_equal(dist_f, dist_o) and np.array_equal(nh_f[:, :, :w], nh_o[:, :, :w]), "oracle vs checker"
    for lo in range(0, len(names), 1040):
        rows = list(range(lo, min(len(names), lo + 1040)))
        dist_f, nh_f = fc.spf_rows([ids[names[i]] for i in rows], [], 16)
        _compare_rows(sw, names, rows, dist_f, nh_f, "checker")


def test_grid13_hop_dist_off(hip, grid13, monkeypatch):
    """ORH_HOP_DIST=0: ms_finalize_kernel writes the distance rows and the
    8-node kernel the masks alone; same rows."""
    monkeypatch.setenv("ORH_HOP_DIST", "0")
    _sweep(hip, grid13, _case_grid13(grid13), 8, 0)


def test_wheel_hop_dist_off(hip, wheel, monkeypatch):
    monkeypatch.setenv("ORH_HOP_DIST", "0")
    _sweep(hip, wheel, _case_wheel(wheel), 8, 0)


_CHILD = r"""
import os, sys
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
import numpy as np
from openr_amd import host_backend
from openr_amd.facade import load_topology
from openr_amd.topology import ladder
from openr_amd.types import K_TESTING_AREA as A
from test_gpu_hop_dist import _wheel
from test_gpu_hop_wide import _defect_grid
hip = host_backend()
out = {}
for tag, dbs, rep in (("grid13", _defect_grid(13), 49), ("wheel", _wheel(), 102), ("ladder", ladder(300, 1)[0], 14)):
    als, _ = load_topology(hip, dbs, [])
    ls = als[A]._impl
    names = sorted(db.thisNodeName for db in dbs) * rep
    sw = ls.sweep(names, True)
    sw.run()
    sw.sync()
    info = sw.info()
    rows = [sw.fetch(i) for i in range(len(names))]
    out[tag + "_dist"] = np.stack([r[0] for r in rows])
    out[tag + "_nh"] = np.stack([r[1] for r in rows])
    out[tag + "_info"] = np.array([info[k] for k in ("variant", "hop_nodes", "hop_dist", "hop_split", "ms_direct", "rows")])
    out[tag + "_words"] = np.array(sw.words)
np.savez(sys.argv[2], **out)
"""


class _Fetched:
    """Rows a child process fetched, behind the sweep interface _compare_rows
    reads."""

    def __init__(self, dist, nh, words):
        self.dist, self.nh, self.words = dist, nh, words

    def fetch(self, i):
        return self.dist[i], self.nh[i]


def test_sixteen_nodes_per_thread(grid13, wheel, ladder300, tmp_path):
    """first_hop_lvl_kernel<16> (ORH_HOP_NODES=16, read once per process,
    hence one fresh child): the 13x13, wheel and ladder sweeps again, every
    row against the same tables."""
    out = tmp_path / "rows.npz"
    env = dict(os.environ, ORH_HOP_NODES="16", ORH_BFS_NH_MAX="0")
    for k in ("ORH_HOP_DIST", "ORH_MS_ORDER", "ORH_MS_BLOCK", "ORH_MS_LATENCY", "ORH_MS_SKIP", "ORH_MS_DIRECT",
              "ORH_MS_WIDE", "ORH_HOP_NARROW"):
        env.pop(k, None)
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out)], check=True, env=env, timeout=120)
    got = np.load(out)
    for tag, g, rep, words in (("grid13", grid13, 49, 1), ("wheel", wheel, 102, 2), ("ladder", ladder300, 14, 1)):
        srcs = g["names"] * rep
        assert _hop_shape(len(g["order"]), len(srcs), 16) == (16, 1, 1)
        # variant, hop_nodes, hop_dist, hop_split, ms_direct, rows
        assert got[tag + "_info"].tolist() == [MSBFS, 16, 1, 1, 0, len(srcs)], tag
        assert int(got[tag + "_words"]) == words
        assert got[tag + "_dist"].shape == (len(srcs), len(g["order"]))
        _check_rows(_Fetched(got[tag + "_dist"], got[tag + "_nh"], words), g, srcs)
