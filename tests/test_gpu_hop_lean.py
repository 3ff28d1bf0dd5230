"""first_hop_lean_kernel, the lean form of the level-row first-hop pass, at the
edges of its preconditions, tiles and redo list: every case sweeps all
sources, and every row - dist and every first-hop mask word - is compared
with the faithful oracle's runSpf tables (LinkState.cpp:808-882).

launch_first_hop keeps the generic kernel's rule for a large batch
(ceil(N / 4096) * n_out >= 8192), so a small graph is swept k times over in
one sweep, as in test_gpu_hop_wide (sources may repeat; the oracle's tables
cover the unique ones, every row is compared). The lean tile is 256 x 4 x Q
nodes with Q = 2: 2,048, the 8-node generic kernel's, and sweep.info()
reports that geometry (hop_nodes 8). ORH_BFS_NH_MAX=0 keeps the sweeps on the
MS-BFS plan; ORH_HOP_LEAN is read per run.

  graph (N)             rows               what the lean kernel meets
  12x12 144             all x 57           one partial tile, aligned rows; the
                                           same sweep under ORH_HOP_LEAN=0 is
                                           byte-identical
  13x13 169             all x 49           N % 4 != 0: declined (hop_lean 0)
  44x44 1936            all x 5            just under one full tile
  45x45 2025            all x 5            N % 4 != 0 again: declined
  46x46 2116            all x 4            one full tile and 68 nodes
  66x66 4356            all x 2            3 tiles walked by one workgroup:
                                           the prefetch's steady state and
                                           its last tile
  12x12 + defects       all x 57           an overloaded neighbour (no
                                           transit), a drained link, an
                                           isolated node (255 bytes, kInf)
  ladder 2x300 600      all x 14           depth > 254: deep sources through
                                           the redo list, both node orders;
                                           then 12x12 and the ladder again on
                                           the same context
  hub of 8 / 9 / wheel  all x k            rank 7 lean; 9 neighbours and two
                                           mask words generic
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid, int_topology, ladder
from openr_amd.types import K_TESTING_AREA
from test_gpu_hop_dist import _wheel
from test_gpu_hop_wide import _check_rows, _defect_grid, _graph

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
MSBFS = 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _ms_bfs_plan(monkeypatch):
    monkeypatch.setenv("ORH_BFS_NH_MAX", "0")
    for k in ("ORH_HOP_LEAN", "ORH_HOP_DIST", "ORH_MS_ORDER", "ORH_MS_BLOCK", "ORH_MS_LATENCY", "ORH_MS_SKIP",
              "ORH_MS_DIRECT", "ORH_MS_WIDE"):
        monkeypatch.delenv(k, raising=False)


def _times(n):
    """Repeats that make a sweep of an n-node graph's sources a large batch."""
    return -(-8192 // (n * -(-n // 4096)))


def _sweep(hip, g, lean, times=None, hop_dist=1, ms_direct=0, check=True):
    """All sources, `times` over, in one sweep on a fresh device mirror: the
    kernel choice from sweep.info(), then every row."""
    als_h, _ = load_topology(hip, g["dbs"], [])
    ls = als_h[A]._impl
    assert ls.node_names() == g["order"]
    srcs = g["names"] * (times or _times(len(g["order"])))
    assert len(srcs) * -(-len(g["order"]) // 4096) >= 8192
    sw = ls.sweep(srcs, True)
    sw.run()
    sw.sync()
    info = sw.info()
    assert info["variant"] == MSBFS and info["rows"] == len(srcs), info
    assert info["hop_lean"] == lean and info["hop_nodes"] == 8, info
    assert info["hop_redo"] == (len(srcs) if lean else 0), info
    assert info["hop_dist"] == hop_dist and info["ms_direct"] == ms_direct, info
    if check:
        _check_rows(sw, g, srcs)
    return sw, srcs


def _rows(sw, n):
    rows = [sw.fetch(i) for i in range(n)]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


@pytest.fixture(scope="module")
def grid12(hip, oracle):
    return _graph(hip, oracle, bench_grid(12)[0])


@pytest.fixture(scope="module")
def ladder300(hip, oracle):
    return _graph(hip, oracle, ladder(300, 1)[0])


def test_grid12_lean_and_generic_identical(hip, grid12, monkeypatch):
    """N = 144: one partial tile (lanes past N load and store nothing), every
    row base 16-byte aligned. The generic kernel's rows are the same bytes."""
    sw, srcs = _sweep(hip, grid12, 1)
    assert len(srcs) == 144 * 57
    lean = _rows(sw, len(srcs))
    monkeypatch.setenv("ORH_HOP_LEAN", "0")
    sw0, _ = _sweep(hip, grid12, 0, check=False)
    generic = _rows(sw0, len(srcs))
    assert np.array_equal(lean[0], generic[0]) and np.array_equal(lean[1], generic[1])


@pytest.mark.parametrize("n,lean", [(13, 0), (44, 1), (45, 0), (46, 1)])
def test_tile_edges_and_odd_sizes(hip, oracle, n, lean):
    """N % 4 != 0 (odd rows' bases off a 16-byte boundary, level-row padding
    inside a lane's dword) is declined: 13x13 and 45x45 run the generic
    kernel. 44x44 and 46x46 are the square grids with N % 4 == 0 on either
    side of one full 2,048-node tile."""
    g = _graph(hip, oracle, bench_grid(n)[0])
    assert (len(g["order"]) % 4 == 0) == bool(lean)
    if n >= 44:
        assert (len(g["order"]) > 2048) == (n == 46)
    _sweep(hip, g, lean)


def test_three_tiles_one_workgroup(hip, oracle):
    """N = 4,356, 8,712 rows: hop_split 1, so a workgroup walks tiles 0, 1 and
    2 (260 nodes): a prefetched tile consumed while the next is in flight,
    and a last tile with nothing behind it."""
    g = _graph(hip, oracle, bench_grid(66)[0])
    sw, srcs = _sweep(hip, g, 1, times=2)
    assert len(g["order"]) == 4356 and len(srcs) == 8712 and sw.info()["hop_split"] == 1


def test_grid12_overloaded_drained_isolated(hip, oracle):
    """Node 40 overloaded (its neighbours' entries skip the transit test but
    keep the direct bit), link 66-67 drained, node 100 isolated (255 level
    bytes -> kInf, no mask bits; its own sweep reaches nothing)."""
    g = _graph(hip, oracle, _defect_grid(12))
    assert np.all((g["dist"] == 0xFFFFFFFF).sum(axis=1) >= 1)
    _sweep(hip, g, 1)


@pytest.mark.parametrize("order", ["cm", "host"])
def test_ladder_deep_sources_redo(hip, ladder300, grid12, monkeypatch, order):
    """Depth 300 > 254: the batches that search that far flag their rows, the
    lean kernel lists the sources that read a flagged row and the generic
    kernel redoes them; the batches in the middle of the ladder stay lean.
    ORH_MS_ORDER=host: the rows come out of the search kernel (ms_direct),
    which sets the flags on that path too. Then, on the same context, a
    shallow sweep (no stale flag or count may redo or skip a source) and the
    ladder again, identical to the first."""
    direct = 0
    if order == "host":
        monkeypatch.setenv("ORH_MS_ORDER", "host")
        direct = 1
    finite = np.where(ladder300["dist"] == 0xFFFFFFFF, 0, ladder300["dist"])
    assert (finite.max(axis=1) >= 254).any() and (finite.max(axis=1) < 254).any()
    hop_dist = 0 if direct else 1
    sw, srcs = _sweep(hip, ladder300, 1, hop_dist=hop_dist, ms_direct=direct)
    first = _rows(sw, len(srcs))
    _sweep(hip, grid12, 1, hop_dist=hop_dist, ms_direct=direct)
    sw2, _ = _sweep(hip, ladder300, 1, hop_dist=hop_dist, ms_direct=direct, check=False)
    again = _rows(sw2, len(srcs))
    assert np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


def _hub(spokes, extra):
    """Hub 0 with `spokes` distinct neighbours in a ring, an outer node behind
    each, and a tail of `extra` nodes behind the last outer node."""
    adj = {0: list(range(1, spokes + 1))}
    for i in range(1, spokes + 1):
        adj[i] = [0, i % spokes + 1, (i - 2) % spokes + 1, spokes + i]
        adj[spokes + i] = [i]
    last = 2 * spokes
    for t in range(extra):
        adj[last].append(last + 1)
        adj[last + 1] = [last]
        last += 1
    return int_topology(adj)


def test_rank_boundary(hip, oracle):
    """Ranks 0..7 fit the packed byte: a hub of exactly 8 distinct neighbours
    is lean. Nine are not (max_nbr > 8), nor is the 40-neighbour wheel's two
    mask words. All three with N % 4 == 0 or, the wheel, 81."""
    g8 = _graph(hip, oracle, _hub(8, 3))
    assert len(g8["order"]) == 20 and max(len(v) for v in g8["nbrs"].values()) == 8
    hub = g8["nh"][g8["at"]["0"]]
    assert (hub[:, 0] & 0x80).any()  # rank 7 is some node's first hop
    _sweep(hip, g8, 1)
    g9 = _graph(hip, oracle, _hub(9, 1))
    assert len(g9["order"]) == 20 and max(len(v) for v in g9["nbrs"].values()) == 9
    _sweep(hip, g9, 0)
    _sweep(hip, _graph(hip, oracle, _wheel()), 0)


def test_hop_dist_off(hip, grid12, monkeypatch):
    """ORH_HOP_DIST=0: ms_finalize_kernel writes the distance rows and the
    lean kernel the masks alone."""
    monkeypatch.setenv("ORH_HOP_DIST", "0")
    _sweep(hip, grid12, 1, hop_dist=0)


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
names = sorted(db.thisNodeName for db in dbs) * 57
sweeps = [ls.sweep(names, True) for _ in range(3)]
for sw in sweeps:  # back to back: both halves of the deferred state in flight
    sw.run()
sweeps[-1].sync()
info = sweeps[-1].info()
out = {k: np.array(info[k]) for k in ("hop_lean", "hop_dist", "variant", "hop_redo")}
for k, sw in enumerate(sweeps):
    rows = [sw.fetch(i) for i in range(len(names))]
    out[f"dist{k}"] = np.stack([r[0] for r in rows])
    out[f"nh{k}"] = np.stack([r[1] for r in rows])
np.savez(sys.argv[2], **out)
"""


def test_deferred_phase2(grid12, tmp_path):
    """ORH_MS_DEFER=1 (read once per process, hence the child): the lean
    kernel and its redo pass on the second stream, flags, list and count per
    half; three sweeps back to back, every row of each exact."""
    out = tmp_path / "rows.npz"
    env = dict(os.environ, ORH_MS_DEFER="1", ORH_BFS_NH_MAX="0")
    for k in ("ORH_HOP_LEAN", "ORH_HOP_DIST", "ORH_MS_ORDER"):
        env.pop(k, None)
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out)], check=True, env=env, timeout=120)
    got = np.load(out)
    assert int(got["variant"]) == MSBFS and int(got["hop_dist"]) == 1
    assert int(got["hop_lean"]) == 1 and int(got["hop_redo"]) == 144 * 57
    g = grid12
    at = [g["at"][s] for s in g["names"] * 57]
    for k in range(3):
        assert np.array_equal(got[f"dist{k}"], g["dist"][at]), k
        nh = got[f"nh{k}"].reshape(len(at), 144, -1)
        w = min(nh.shape[2], g["nh"].shape[2])
        assert np.array_equal(nh[:, :, :w], g["nh"][at][:, :, :w]), k
        assert not nh[:, :, w:].any() and not g["nh"][:, :, w:].any()
