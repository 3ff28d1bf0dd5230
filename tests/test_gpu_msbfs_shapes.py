"""Every spf_msbfs_kernel<K, M, J, kSkip> shape launch_ms_m can pick, each
under a plan that does not depend on what else the device is running, every
checked row - dist and every first-hop mask word - exact against the
faithful oracle's runSpf tables (LinkState.cpp:808-882).

ORH_MS_BLOCK (read on every plan) fixes the threads per workgroup and turns
the latency and lone-sweep plans off, so J = 4 * ceil(ceil(N / block) / 4) is
a function of N alone; ORH_BFS_NH_MAX=0 (read per run) keeps small sweeps off
the fused per-source BFS.

  matrix   J in {4, ..., 32} x K in {4, 8} x node order {cm, host} at 64
           threads: N = 64 * J - 37 (a partial last chunk, N % 16 != 0), a
           ring with seeded short chords (BFS depth > 32) and one hub of 14
           neighbours (a continuation record at either K); 96 sources, so
           neighbour-only rows are present; all 96 rows compared.
           J = 32 is the end of the arrival log's 11-bit node field, and its
           log-assembly LDS (32 * 64 * 36 = 73,728 B) exceeds the frontier
           arrays: launch_ms_j's max and the dynamic-LDS opt-in past 64 KB
  skip     J in {8, 28, 32}, K = 4 again with ORH_MS_SKIP=1 (kSkip = true)
  2 waves  J = 16 at 128 threads on N = 2,011: the per-wave log loop twice
  natural  the two J = 32 plans of the default planner, ORH_MS_LATENCY=0:
           127x127 grid (N = 16,129): 512 threads, u32 masks
           150x150 grid (N = 22,500): 768 threads, u16 masks
           20 rows compared in full each
"""
import random

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid, int_topology
from openr_amd.types import K_TESTING_AREA
from test_gpu_weighted import _compare_rows

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
MSBFS = 1
INF = 0xFFFFFFFF
N_SOURCES = 96
JS = [4, 8, 12, 16, 20, 24, 28, 32]


@pytest.fixture(autouse=True)
def _deterministic_plan(monkeypatch):
    monkeypatch.setenv("ORH_BFS_NH_MAX", "0")
    for k in ("ORH_MS_BLOCK", "ORH_MS_LATENCY", "ORH_MS_SKIP", "ORH_MS_ORDER", "ORH_MS_DIRECT",
              "ORH_MS_WIDE", "ORH_HOP_DIST"):
        monkeypatch.delenv(k, raising=False)


def _ceil(a, b):
    return -(-a // b)


def _ms_j(n, block):
    """plan_spf's J: nodes per thread, rounded up to a multiple of 4."""
    return 4 * _ceil(_ceil(n, block), 4)


def _ell_k(dbs):
    """choose_ell_k restated: 8 when the 90th-percentile out-degree passes 4
    (the info record does not report K)."""
    deg = sorted(len(db.adjacencies) for db in dbs)
    return 8 if deg[len(deg) * 9 // 10] > 4 else 4


def _ring_with_chords(n, k):
    """A ring 0..n-1 (k = 8: every node also linked two apart, degree >= 4),
    seeded chords no longer than max(base + 1, n / 80) <= n / 16 - short
    enough that the BFS stays deep - and a hub linked to its 7 nearest nodes
    on either side. k = 4: n / 8 chords, so most nodes keep degree 2..4;
    k = 8: n / 3 chords, so about half the nodes have degree >= 5."""
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
    assert cap <= n // 16
    for _ in range(n // 8 if k == 4 else n // 3):
        a = rng.randrange(n)
        link(a, (a + rng.randint(base + 1, cap)) % n)
    hub = n // 2
    for d in range(1, 8):
        link(hub, hub + d)
        link(hub, hub - d)
    return adj, hub


@pytest.fixture(scope="module")
def matrix(hip, oracle):
    """(n, k) -> the graph, its 96 seeded sources and their oracle tables,
    computed once and shared by every parameter that runs the graph."""
    memo = {}

    def get(n, k):
        if (n, k) in memo:
            return memo[(n, k)]
        adj, hub = _ring_with_chords(n, k)
        dbs = int_topology(adj)
        assert _ell_k(dbs) == k
        assert len(set(adj[hub])) >= 12  # past either ELL width: a continuation record
        rng = random.Random(n + k)
        srcs = [str(hub)] + [str(v) for v in rng.sample([v for v in range(n) if v != hub], N_SOURCES - 1)]
        als_h, _ = load_topology(hip, dbs, [])
        als_o, _ = load_topology(oracle, dbs, [])
        ls = als_h[A]._impl
        order = ls.node_names()
        nbrs = [ls.neighbors(s) for s in srcs]
        dist_o, nh_o = als_o[A]._impl.spf_tables(srcs, order, nbrs, 16)
        dist_o.setflags(write=False)
        nh_o.setflags(write=False)
        assert not (dist_o == INF).any()
        assert int(dist_o.max()) > 32  # BFS depth, from the CPU tables
        memo[(n, k)] = {"dbs": dbs, "srcs": srcs, "order": order, "nbrs": nbrs, "dist": dist_o, "nh": nh_o}
        return memo[(n, k)]

    return get


def _run(hip, g, block, j, order="cm", skip=0):
    """One sweep of the graph's sources on a fresh device mirror (the layout
    reads ORH_MS_ORDER and ORH_MS_SKIP, so the environment is set first), the
    kernel shape from sweep.info(), all rows compared."""
    n = len(g["order"])
    assert _ms_j(n, block) == j
    als_h, _ = load_topology(hip, g["dbs"], [])
    ls = als_h[A]._impl
    assert ls.node_names() == g["order"]
    assert [ls.neighbors(s) for s in g["srcs"]] == g["nbrs"]
    sw = ls.sweep(g["srcs"], True)
    sw.run()
    sw.sync()
    info = sw.info()
    assert info["variant"] == MSBFS, info
    assert info["ms_threads"] == block and info["mask_bits"] == 32, info
    assert info["ms_direct"] == (1 if order == "host" else 0), info
    assert info["ms_skip"] == skip, info
    assert info["rows"] > len(g["srcs"]), info  # neighbour-only rows
    _compare_rows(sw, g["srcs"], list(range(len(g["srcs"]))), g["dist"], g["nh"], "oracle")
    return info


@pytest.mark.parametrize("order", ["cm", "host"])
@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("j", JS)
def test_matrix_j_k_order(hip, matrix, monkeypatch, j, k, order):
    """spf_msbfs_kernel<k, u32, j, false> at 64 threads, rows through
    ms_finalize_kernel (cm) and out of the search kernel (host)."""
    monkeypatch.setenv("ORH_MS_BLOCK", "64")
    monkeypatch.setenv("ORH_MS_ORDER", order)
    n = 64 * j - 37
    assert n % 16 != 0 and _ceil(n, 64) == j and n % 64 != 0
    _run(hip, matrix(n, k), 64, j, order)


@pytest.mark.parametrize("j", [8, 28, 32])
def test_matrix_interval_skip(hip, matrix, monkeypatch, j):
    """spf_msbfs_kernel<4, u32, j, true>: the interval skip over slices out of
    reach of the previous level's frontier."""
    monkeypatch.setenv("ORH_MS_BLOCK", "64")
    monkeypatch.setenv("ORH_MS_SKIP", "1")
    _run(hip, matrix(64 * j - 37, 4), 64, j, skip=1)


def test_two_waves_j16(hip, matrix, monkeypatch):
    """N = 2,011 at 128 threads: J = 16, and the log assembly's per-wave loop
    runs twice."""
    monkeypatch.setenv("ORH_MS_BLOCK", "128")
    _run(hip, matrix(2011, 4), 128, 16)


def _natural(hip, oracle, n, names, check, threads, mask_bits):
    """A grid sweep under the default planner with the latency and lone-sweep
    plans off; rows `check` (indices into names) against the oracle."""
    dbs, _ = bench_grid(n)
    als_h, _ = load_topology(hip, dbs, [])
    als_o, _ = load_topology(oracle, dbs, [])
    ls = als_h[A]._impl
    assert _ms_j(n * n, threads) == 32
    sw = ls.sweep(names, True)
    sw.run()
    sw.sync()
    info = sw.info()
    assert info["variant"] == MSBFS, info
    assert info["ms_threads"] == threads and info["mask_bits"] == mask_bits, info
    assert info["ms_direct"] == 0 and info["ms_skip"] == 0, info
    assert len(check) == 20
    srcs = [names[i] for i in check]
    dist_o, nh_o = als_o[A]._impl.spf_tables(srcs, ls.node_names(), [ls.neighbors(s) for s in srcs], 16)
    _compare_rows(sw, names, check, dist_o, nh_o, "oracle")


def test_natural_j32_512_threads_127x127(hip, oracle, monkeypatch):
    """N = 16,129 (14,337..16,368 nodes): the base plan's 512 threads need
    J = 32 with u32 masks. 16 seeded sources and the four corners, every row
    compared."""
    monkeypatch.setenv("ORH_MS_LATENCY", "0")
    n = 127
    corners = [0, n - 1, n * (n - 1), n * n - 1]
    rng = random.Random(127)
    names = [str(v) for v in corners + rng.sample([v for v in range(n * n) if v not in corners], 16)]
    _natural(hip, oracle, n, names, list(range(20)), 512, 32)


def test_natural_j32_768_threads_150x150(hip, oracle, monkeypatch):
    """N = 22,500 under the base plan (768 threads, u16 masks, J = 32; the
    latency plan would take 1,024 threads and J = 24): the source list of
    test_gpu_configs.test_u16_mask_msbfs_150x150, 20 rows compared."""
    monkeypatch.setenv("ORH_MS_LATENCY", "0")
    n = 150
    names = [str(i) for i in range(0, n * n, 37)] + [str(n * n - 1)]
    rng = random.Random(150)
    check = [0, len(names) - 1] + rng.sample(range(1, len(names) - 1), 18)
    _natural(hip, oracle, n, names, check, 768, 16)
