"""MS-BFS sweeps whose u32 distance rows are written by the first-hop pass
(first_hop_lvl_kernel with HopArgs::write_dist) after a level-only
ms_finalize_kernel (info["hop_dist"] == 1), and the sweeps that keep the rows
in ms_finalize_kernel or the search kernel (hop_dist == 0): every row - dist
and every first-hop mask word - against the faithful oracle's runSpf tables
(LinkState.cpp:808-882).

Small sweeps take the fused per-source BFS by default; ORH_BFS_NH_MAX=0 (read
per run) sends them through the MS-BFS plan under test.

  grid 12x12   N = 144: one partial 256-node finalize tile, one partial
               first-hop tile, every row base 16-byte aligned (vector stores)
  grid 13x13   N = 169: level-row padding [169, 176), a tile that ends past N
               and odd rows' bases off a 16-byte boundary (per-element stores)
  drained      the 12x12 grid with an overloaded node, a drained link and an
               isolated node (255 level bytes, kInf entries)
  ladder 2x300 BFS depth > 254: the kLvlDirect entries keep the search
               kernel's values
  wheel        a hub of 40 distinct neighbours: two mask words per node, the
               row written once per tile, not once per word
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid, int_topology, ladder
from openr_amd.types import K_TESTING_AREA
from test_gpu_weighted import _compare_rows

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
MSBFS = 1
INF = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _ms_bfs_plan(monkeypatch):
    monkeypatch.setenv("ORH_BFS_NH_MAX", "0")
    monkeypatch.delenv("ORH_HOP_DIST", raising=False)
    monkeypatch.delenv("ORH_MS_ORDER", raising=False)


def _names(dbs):
    return sorted(db.thisNodeName for db in dbs)


def _oracle_tables(oracle, ls, dbs):
    """The oracle's dist / first-hop tables of every node as a source, in the
    product's node and neighbour order; read-only, shared."""
    als_o, _ = load_topology(oracle, dbs, [])
    names = _names(dbs)
    dist_o, nh_o = als_o[A]._impl.spf_tables(names, ls.node_names(), [ls.neighbors(s) for s in names], 16)
    dist_o.setflags(write=False)
    nh_o.setflags(write=False)
    return dist_o, nh_o


def _sweep_all(hip, dbs, dist_o, nh_o, hop_dist, ms_direct=0):
    """All sources in one sweep on a fresh device mirror, every row compared."""
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    names = _names(dbs)
    sw = ls.sweep(names, True)
    sw.run()
    sw.sync()
    info = sw.info()
    assert info["variant"] == MSBFS and info["ms_direct"] == ms_direct, info
    assert info["hop_dist"] == hop_dist, info
    _compare_rows(sw, names, list(range(len(names))), dist_o, nh_o, "oracle")
    return sw, info, ls


def _case(hip, oracle, dbs, hop_dist=1):
    als_h, _ = load_topology(hip, dbs, [])
    dist_o, nh_o = _oracle_tables(oracle, als_h[A]._impl, dbs)
    sw, info, ls = _sweep_all(hip, dbs, dist_o, nh_o, hop_dist)
    return sw, info, ls, dist_o, nh_o


@pytest.fixture(scope="module")
def grid12(hip, oracle):
    dbs, _ = bench_grid(12)
    als_h, _ = load_topology(hip, dbs, [])
    dist_o, nh_o = _oracle_tables(oracle, als_h[A]._impl, dbs)
    return {"dbs": dbs, "dist": dist_o, "nh": nh_o}


def test_grid_12x12_all_sources(hip, grid12):
    """N = 144 (no multiple of 256 or of 16 x 64): tail tiles; the source's
    own entry is distance 0 with no first hops."""
    g = grid12
    sw, info, ls = _sweep_all(hip, g["dbs"], g["dist"], g["nh"], 1)
    assert info["hop_nodes"] == 4 and info["mask_bits"] == 32, info
    order = ls.node_names()
    for i, s in enumerate(_names(g["dbs"])):
        d, m = sw.fetch(i)
        at = order.index(s)
        assert d[at] == 0 and not m.reshape(len(order), -1)[at].any(), s
    assert int(g["dist"].max()) == 22


def test_grid_12x12_overloaded_drained_isolated(hip, oracle, grid12):
    """An overloaded node (reached, no transit), a drained link and a node
    isolated by draining its four links: unreached entries (level byte 255 ->
    kInf) in every row, and the isolated source's row unreached but for
    itself."""
    dbs, _ = bench_grid(12)
    dbs[40].isOverloaded = True
    for x in (66, 100):
        for adj in dbs[x].adjacencies:
            if x == 100 or adj.otherNodeName == "67":
                adj.isOverloaded = True
                for back in dbs[int(adj.otherNodeName)].adjacencies:
                    if back.otherNodeName == str(x):
                        back.isOverloaded = True
    sw, info, ls, dist_o, _ = _case(hip, oracle, dbs)
    names, order = _names(dbs), ls.node_names()
    assert np.all((dist_o == INF).sum(axis=1) >= 1)
    row = dist_o[names.index("100")]
    assert (row == INF).sum() == 143 and row[order.index("100")] == 0
    assert not np.array_equal(dist_o, grid12["dist"])  # the detours lengthen paths


def test_ladder_deep_levels_all_sources(hip, oracle):
    """A 2 x 300 ladder: levels >= 254 (kLvlDirect) are written by the search
    kernel and skipped by the first-hop pass's row stores; sources at both
    ends and in the middle among all 600."""
    dbs, _ = ladder(300, 1)
    sw, info, ls, dist_o, _ = _case(hip, oracle, dbs)
    assert info["hop_nodes"] == 4, info
    names = _names(dbs)
    finite = np.where(dist_o == INF, 0, dist_o)
    assert int(finite.max()) == 300 > 254  # the graph's diameter, from the CPU tables
    for s, deepest in (("a0", 300), ("b299", 300), ("a150", 151)):
        row = finite[names.index(s)]
        assert int(row.max()) == deepest, s
    # rows with and without deep entries both occur
    assert (finite.max(axis=1) >= 254).any() and (finite.max(axis=1) < 254).any()


def _wheel():
    """Hub 0 with 40 spokes 1..40 in a ring, and an outer ring 41..80 whose
    node 40 + i hangs off spokes i and i + 1 (two equal-cost first hops)."""
    adj = {0: list(range(1, 41))}
    for i in range(1, 41):
        nxt, prv = i % 40 + 1, (i - 2) % 40 + 1
        adj[i] = [0, nxt, prv, 40 + i, 40 + prv]
    for i in range(1, 41):
        adj[40 + i] = [i, i % 40 + 1]
    return int_topology(adj)


def test_two_mask_words(hip, oracle):
    """A source of 40 distinct neighbours: every node carries two mask words,
    and the distance row is written once per tile whatever the word count."""
    dbs = _wheel()
    sw, info, ls, dist_o, nh_o = _case(hip, oracle, dbs)
    assert sw.words == 2 and nh_o.shape[2] >= 2
    hub = nh_o[_names(dbs).index("0")]
    assert hub[:, 0].any() and hub[:, 1].any()  # first hops of rank >= 32 occur
    assert int(dist_o.max()) == 4


def test_grid_13x13_odd_n(hip, oracle):
    """N = 169: the rows of odd sources start off a 16-byte boundary (per-
    element stores), and the level rows are padded to 176."""
    dbs, _ = bench_grid(13)
    sw, info, _, dist_o, _ = _case(hip, oracle, dbs)
    assert sw.nodes == 169 and info["hop_nodes"] == 4, info


def test_hop_dist_off_same_rows(hip, grid12, monkeypatch):
    """ORH_HOP_DIST=0: ms_finalize_kernel writes the distance rows, as before."""
    monkeypatch.setenv("ORH_HOP_DIST", "0")
    g = grid12
    _sweep_all(hip, g["dbs"], g["dist"], g["nh"], 0)


def test_host_order_rows_stay_in_search_kernel(hip, grid12, monkeypatch):
    """ORH_MS_ORDER=host (ms_direct): the search kernel writes the rows and no
    finalize pass runs, so the first-hop pass leaves them alone."""
    monkeypatch.setenv("ORH_MS_ORDER", "host")
    g = grid12
    _sweep_all(hip, g["dbs"], g["dist"], g["nh"], 0, ms_direct=1)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from openr_amd import host_backend
from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid
from openr_amd.types import K_TESTING_AREA as A
dbs, _ = bench_grid(12)
als, _ = load_topology(host_backend(), dbs, [])
ls = als[A]._impl
names = sorted(db.thisNodeName for db in dbs)
sweeps = [ls.sweep(names, True) for _ in range(3)]
for sw in sweeps:  # back to back: both halves of the deferred scratch in flight
    sw.run()
sweeps[-1].sync()
info = sweeps[-1].info()
out = {"hop_dist": np.array(info["hop_dist"]), "variant": np.array(info["variant"])}
for k, sw in enumerate(sweeps):
    rows = [sw.fetch(i) for i in range(len(names))]
    out[f"dist{k}"] = np.stack([r[0] for r in rows])
    out[f"nh{k}"] = np.stack([r[1] for r in rows])
np.savez(sys.argv[2], **out)
"""


def test_deferred_phase2(grid12, tmp_path):
    """ORH_MS_DEFER=1 (read once per process, hence the child): finalize and
    first hops of a sweep run on the second stream; three sweeps back to back,
    every row of each exact."""
    out = tmp_path / "rows.npz"
    env = dict(os.environ, ORH_MS_DEFER="1", ORH_BFS_NH_MAX="0")
    env.pop("ORH_HOP_DIST", None)
    env.pop("ORH_MS_ORDER", None)
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out)], check=True, env=env, timeout=120)
    got = np.load(out)
    assert int(got["variant"]) == MSBFS and int(got["hop_dist"]) == 1
    g = grid12
    n = g["dist"].shape[0]
    for k in range(3):
        assert np.array_equal(got[f"dist{k}"], g["dist"]), k
        nh = got[f"nh{k}"].reshape(n, n, -1)
        w = min(nh.shape[2], g["nh"].shape[2])
        assert np.array_equal(nh[:, :, :w], g["nh"][:, :, :w]), k
        assert not nh[:, :, w:].any() and not g["nh"][:, :, w:].any()
