"""Which plan orh_spf_run picks, case by case: one sweep through
LinkState.sweep per case, the plan it reports (orh_last_spf_info: variant,
rows, mask_bits, batch_sources, ms_threads, ms_skip, ms_direct, hop_dist,
hop_nodes, hop_split) compared field by field, and every row - dist and every
first-hop mask word - against the faithful oracle's runSpf tables
(LinkState.cpp:808-882).

The shapes are the smallest at which each rule of the plan choice still has
something to decide:

  grid 12x12    uniform, N = 144 < 255: BFS_NH / MSBFS by ORH_BFS_NH_MAX, BFS8,
                GLOBAL_NH and GLOBAL by orh_set_spf_mode
  grid 17x17    uniform, N = 289 >= 255: BFS16, with neighbour rows
  random 250    metrics 1..9, at most 32 neighbours: two-phase DIST16 below
                ORH_LDS_NH_MIN sources, LDS_NH from there, DIST32 with the
                metrics scaled past a 16-bit path bound
  ring 300      seeded chords, every degree <= 8, all sources (>= ORH_WMS_MIN): WMS
  clos 400      FSWs of 84 neighbours, all sources: WMS_SLICED, the two-phase
                plan with ORH_WMS_SLICED=0
  zero metric   EXACT
  staging       a repeated request (staged once), then another source list
  deferred      ORH_MS_DEFER=1 (read once per process, hence a child)
"""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from openr_amd import host_module
from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid, int_topology
from openr_amd.types import K_TESTING_AREA
from openr_amd.workloads import c3_weighted_fabric
from test_gpu_parity import random_topology
from test_gpu_weighted import _compare_rows

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# ORH_VARIANT_*
MSBFS, BFS8, BFS16, DIST16, DIST32, GLOBAL, GLOBAL_NH, EXACT, BFS_NH, LDS_NH, WMS, WMS_SLICED = \
    1, 2, 3, 5, 6, 7, 8, 9, 10, 12, 13, 14
PER_SOURCE, GLOBAL_MODE, GLOBAL_TWO_PHASE = 1, 2, 3  # orh_set_spf_mode
FIELDS = ("variant", "rows", "mask_bits", "batch_sources", "ms_threads", "ms_skip", "ms_direct",
          "hop_dist", "hop_nodes", "hop_split")
# every knob read per run, by orh_spf_run or by the planners it calls
KNOBS = ("ORH_BFS_NH_MAX", "ORH_WMS_SLICED", "ORH_WMS_SLICED_ALL", "ORH_WMS_SLICED_BLOCK", "ORH_MS_DIRECT",
         "ORH_WMS_SKIP", "ORH_WMS_BAND", "ORH_HOP_DIST", "ORH_MS_ORDER", "ORH_MS_LATENCY", "ORH_MS_BLOCK",
         "ORH_MS_WIDE", "ORH_MS_SKIP", "ORH_WMS_SOURCES")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _want(variant, rows, **kw):
    """The plan fields of a sweep; the ones not named are 0."""
    d = dict.fromkeys(FIELDS, 0)
    d.update(variant=variant, rows=rows, **kw)
    return d


# the first-hop phase over u32 distance rows: one node per thread, one tile of
# 1,024 nodes (every graph here has fewer)
TWO_PHASE = dict(hop_nodes=1, hop_split=1)
# the multi-source BFS of a graph of <= 1,024 nodes whose batches have a CU
# each: u32 masks, 32 sources per batch, 1,024 threads; Cuthill-McKee order, so
# the rows come from the first-hop pass over the level rows (4 nodes per thread)
MS_SMALL = dict(mask_bits=32, batch_sources=32, ms_threads=1024, hop_dist=1, hop_nodes=4, hop_split=1)


class _Graph:
    """A topology on the HIP backend and the oracle's tables of every node as
    a source (read-only, computed once)."""

    def __init__(self, hip, oracle, dbs):
        self.dbs = dbs
        self.als, _ = load_topology(hip, dbs, [])
        self.ls = self.als[A]._impl
        als_o, _ = load_topology(oracle, dbs, [])
        self.names = sorted(db.thisNodeName for db in dbs)
        self.order = self.ls.node_names()
        self.dist, self.nh = als_o[A]._impl.spf_tables(
            self.names, self.order, [self.ls.neighbors(s) for s in self.names], 16)
        self.dist.setflags(write=False)
        self.nh.setflags(write=False)
        self.at = {s: k for k, s in enumerate(self.names)}

    def rows(self, names):
        """Distance rows of a two-phase sweep: the sources and their distinct
        neighbours, one row per node."""
        return len(set(names) | {u for s in names for u in self.ls.neighbors(s)})

    def max_neighbours(self, names):
        return max(len(self.ls.neighbors(s)) for s in names)

    def sweep(self, names, want, label, mode=0):
        mod = host_module()
        mod.set_spf_mode(mode)
        try:
            sw = self.ls.sweep(names, True)
            sw.run()
            sw.sync()
            info = sw.info()
        finally:
            mod.set_spf_mode(0)
        got = {k: int(info[k]) for k in FIELDS}
        print("plan", label, got)
        assert got == want, (label, got, want)
        idx = [self.at[s] for s in names]
        _compare_rows(sw, names, list(range(len(names))), self.dist[idx], self.nh[idx], label)
        return sw


# ---- uniform metrics --------------------------------------------------------

@pytest.fixture(scope="module")
def grid12(hip, oracle):
    return _Graph(hip, oracle, bench_grid(12)[0])


def test_uniform_default_is_bfs_nh(grid12):
    """144 sources <= one per CU: the fused BFS, one row per source."""
    g = grid12
    g.sweep(g.names, _want(BFS_NH, 144), "grid12 default")


def test_uniform_bfs_nh_off_is_msbfs(grid12, monkeypatch):
    monkeypatch.setenv("ORH_BFS_NH_MAX", "0")
    g = grid12
    g.sweep(g.names, _want(MSBFS, 144, **MS_SMALL), "grid12 ORH_BFS_NH_MAX=0")


def test_uniform_per_source_is_bfs8(grid12):
    g = grid12
    g.sweep(g.names, _want(BFS8, 144, **TWO_PHASE), "grid12 mode 1", mode=PER_SOURCE)


def test_uniform_global_is_global_nh(grid12):
    g = grid12
    g.sweep(g.names, _want(GLOBAL_NH, 144), "grid12 mode 2", mode=GLOBAL_MODE)


def test_uniform_global_two_phase_is_global(grid12):
    g = grid12
    g.sweep(g.names, _want(GLOBAL, 144, **TWO_PHASE), "grid12 mode 3", mode=GLOBAL_TWO_PHASE)


def test_uniform_289_nodes_per_source_is_bfs16(hip, oracle):
    """N = 289 >= 255: u16 levels; 12 seeded sources, so their neighbours that
    are no sources get scratch rows."""
    g = _Graph(hip, oracle, bench_grid(17)[0])
    names = random.Random(21).sample(g.names, 12)
    rows = g.rows(names)
    assert rows > len(names)
    g.sweep(names, _want(BFS16, rows, **TWO_PHASE), "grid17 mode 1", mode=PER_SOURCE)


# ---- general metrics --------------------------------------------------------

def _random250():
    return random_topology(2100, n=250, extra=250, max_metric=9, parallel=0.1, overload=0.05,
                           link_overload=0.02)


@pytest.fixture(scope="module")
def rand250(hip, oracle):
    g = _Graph(hip, oracle, _random250())
    assert g.max_neighbours(g.names) <= 32
    return g


def test_weighted_few_sources_two_phase_dist16(rand250):
    """8 sources < ORH_LDS_NH_MIN: the two-phase LDS plan with neighbour rows."""
    g = rand250
    names = random.Random(22).sample(g.names, 8)
    rows = g.rows(names)
    assert rows > 8
    g.sweep(names, _want(DIST16, rows, **TWO_PHASE), "rand250 8 sources")


def test_weighted_40_sources_lds_nh(rand250):
    g = rand250
    names = random.Random(23).sample(g.names, 40)
    g.sweep(names, _want(LDS_NH, 40), "rand250 40 sources")


def test_weighted_40_sources_per_source_mode_keeps_two_phase(rand250):
    g = rand250
    names = random.Random(23).sample(g.names, 40)
    rows = g.rows(names)
    assert rows > 40
    g.sweep(names, _want(DIST16, rows, **TWO_PHASE), "rand250 40 sources mode 1", mode=PER_SOURCE)


def test_weighted_wide_path_bound_dist32(hip, oracle):
    """The same graph at 1,000 times the metrics: the path bound passes
    0xFFFF, so u32 labels."""
    dbs = _random250()
    for db in dbs:
        for adj in db.adjacencies:
            adj.metric *= 1000
    g = _Graph(hip, oracle, dbs)
    names = random.Random(22).sample(g.names, 8)
    rows = g.rows(names)
    assert rows > 8
    g.sweep(names, _want(DIST32, rows, **TWO_PHASE), "rand250 x1000 8 sources")


def _low_degree_300():
    """A ring of 300 nodes with seeded chords, every degree <= 8 (WMS keeps a
    node's in-links in 8 slots), a seeded metric 1..9 per link."""
    rng = random.Random(2200)
    n = 300
    links = {(i, (i + 1) % n) for i in range(n)}
    deg = [2] * n
    for _ in range(1500):
        a, b = rng.randrange(n), rng.randrange(n)
        if a != b and deg[a] < 8 and deg[b] < 8 and (a, b) not in links and (b, a) not in links:
            links.add((a, b))
            deg[a] += 1
            deg[b] += 1
    adj = {i: [] for i in range(n)}
    for a, b in sorted(links):
        w = rng.randint(1, 9)
        adj[a].append((b, w))
        adj[b].append((a, w))
    assert 4 < max(deg) <= 8
    return int_topology(adj)


@pytest.fixture(scope="module")
def rand300(hip, oracle):
    return _Graph(hip, oracle, _low_degree_300())


@pytest.mark.parametrize("sliced", [None, "0"])
def test_weighted_all_sources_low_degree_wms(rand300, monkeypatch, sliced):
    """All 300 sources (>= ORH_WMS_MIN), every degree <= 8: WMS, whatever
    ORH_WMS_SLICED says."""
    if sliced is not None:
        monkeypatch.setenv("ORH_WMS_SLICED", sliced)
    g = rand300
    g.sweep(g.names, _want(WMS, 300, **TWO_PHASE), f"rand300 all ORH_WMS_SLICED={sliced}")


@pytest.fixture(scope="module")
def clos400(hip, oracle):
    return _Graph(hip, oracle, c3_weighted_fabric(400, 4, 7)[0])


def test_weighted_clos_all_sources_wms_sliced(clos400):
    """FSWs of 84 neighbours: WMS declines, the sliced plan takes the sweep;
    8-source batches at the layout's own workgroup width."""
    g = clos400
    assert g.max_neighbours(g.names) > 32
    g.sweep(g.names, _want(WMS_SLICED, 400, batch_sources=8, ms_threads=256, **TWO_PHASE), "clos400 all")


def test_weighted_clos_sliced_off_two_phase(clos400, monkeypatch):
    monkeypatch.setenv("ORH_WMS_SLICED", "0")
    g = clos400
    g.sweep(g.names, _want(DIST16, 400, **TWO_PHASE), "clos400 all ORH_WMS_SLICED=0")


def test_zero_metric_is_exact(hip, oracle):
    g = _Graph(hip, oracle, random_topology(1300, n=64, extra=120, min_metric=0, max_metric=4))
    g.sweep(g.names, _want(EXACT, 64), "zero metric")


def test_staged_request_hit_then_miss(rand250):
    """Three identical sweeps (the request staged once, then reused) and one
    with another source list on the same graph (staged anew)."""
    g = rand250
    rng = random.Random(24)
    first, other = rng.sample(g.names, 8), rng.sample(g.names, 11)
    assert first != other
    for k in range(3):
        g.sweep(first, _want(DIST16, g.rows(first), **TWO_PHASE), f"staging repeat {k}")
    g.sweep(other, _want(DIST16, g.rows(other), **TWO_PHASE), "staging other list")


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from openr_amd import host_backend
from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid, int_topology
from openr_amd.types import K_TESTING_AREA as A
dbs, _ = bench_grid(12)
als, _ = load_topology(host_backend(), dbs, [])
ls = als[A]._impl
names = sorted(db.thisNodeName for db in dbs)
sw = ls.sweep(names, True)
sw.run()
sw.sync()
info = sw.info()
rows = [sw.fetch(i) for i in range(len(names))]
np.savez(sys.argv[2], dist=np.stack([r[0] for r in rows]), nh=np.stack([r[1] for r in rows]),
         **{k: np.array(int(info[k])) for k in sys.argv[3].split(",")})
"""


def test_deferred_phase2(grid12, tmp_path):
    """ORH_MS_DEFER=1: an ORH_SPF_DEFER_HOPS sweep (every LinkState.sweep is
    one) runs finalize and first hops on the second stream."""
    out = tmp_path / "rows.npz"
    env = dict(os.environ, ORH_MS_DEFER="1", ORH_BFS_NH_MAX="0")
    for k in KNOBS:
        if k != "ORH_BFS_NH_MAX":
            env.pop(k, None)
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out), ",".join(FIELDS)], check=True, env=env,
                   timeout=120)
    got = np.load(out)
    plan = {k: int(got[k]) for k in FIELDS}
    print("plan", "grid12 deferred", plan)
    assert plan == _want(MSBFS, 144, **MS_SMALL)
    g = grid12
    assert np.array_equal(got["dist"], g.dist)
    nh = got["nh"].reshape(144, 144, -1)
    w = min(nh.shape[2], g.nh.shape[2])
    assert np.array_equal(nh[:, :, :w], g.nh[:, :, :w])
    assert not nh[:, :, w:].any() and not g.nh[:, :, w:].any()
