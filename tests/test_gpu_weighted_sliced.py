"""Weighted sweeps over graphs with high-degree nodes: the sliced multi-source
Bellman-Ford plan (spf_wms_sliced_kernel, ORH_VARIANT_WMS_SLICED), which takes
the sweeps of >= ORH_WMS_MIN sources whose sources have more than 32 distinct
neighbours (the two-phase per-source plan before), and that older plan, every
row - dist and every first-hop mask word - against the faithful oracle's
runSpf tables (LinkState.cpp:808-882).

  clos400   fabric(400, bug_compatible=False): 288 spines of degree 2, 16 FSWs
            of degree 84, 96 RSWs of degree 8; 3 mask words; seeded metrics
  random    test_gpu_parity.random_topology graphs (degree <= 32) through
            ORH_WMS_SLICED_ALL=1
"""
import copy
import random

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import fabric
from openr_amd.types import K_TESTING_AREA
from openr_amd.workloads import weight_links
from test_gpu_weighted import _compare_rows, _random_weighted

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
DIST16, DIST32, LDS_NH, SLICED = 5, 6, 12, 14  # ORH_VARIANT_*


def _clos400(lo, hi, seed, symmetric):
    dbs, _ = fabric(400, bug_compatible=False)
    return weight_links(dbs, lo, hi, seed, symmetric)


def _oracle_tables(oracle, hip_ls, dbs):
    """(oracle link states, node order, {name: row}, dist, nh) of every node as a source."""
    als_o, _ = load_topology(oracle, dbs, [])
    order = hip_ls.node_names()
    uniq = sorted(db.thisNodeName for db in dbs)
    dist_o, nh_o = als_o[A]._impl.spf_tables(uniq, order, [hip_ls.neighbors(s) for s in uniq], 16)
    return als_o, order, {s: k for k, s in enumerate(uniq)}, dist_o, nh_o


def _sweep(ls, names):
    sw = ls.sweep(names, True)
    sw.run()
    sw.sync()
    return sw, sw.info()


def _check(sw, names, at, dist_o, nh_o):
    idx = [at[s] for s in names]
    _compare_rows(sw, names, list(range(len(names))), dist_o[idx], nh_o[idx], "oracle")


@pytest.fixture(scope="module")
def clos_sym(hip, oracle):
    """Case 1's graph (metrics 1..4, symmetric, seed 7) on both backends, and
    the oracle's tables of all 400 sources, shared by the tests that sweep it."""
    dbs = _clos400(1, 4, 7, True)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    _, order, at, dist_o, nh_o = _oracle_tables(oracle, ls, dbs)
    dist_o.setflags(write=False)
    nh_o.setflags(write=False)
    return {"dbs": dbs, "als": als_h, "ls": ls, "names": sorted(at), "at": at, "dist": dist_o, "nh": nh_o}


def test_symmetric_small_metrics(clos_sym):
    """All 400 sources: the sliced plan, distances first, then every first hop
    from the u32 rows. Not degenerate: 3 mask words, ECMP sets that reach past
    rank 31."""
    c = clos_sym
    sw, info = _sweep(c["ls"], c["names"])
    assert info["variant"] == SLICED and info["rows"] == 400 and info["hop_nodes"] == 1, info
    _check(sw, c["names"], c["at"], c["dist"], c["nh"])
    assert sw.words == 3
    assert int(c["dist"][c["dist"] != 0xFFFFFFFF].max()) == 10
    found = False
    for i in range(0, 400, 7):
        m = sw.fetch(i)[1].reshape(-1, 3)
        bits = np.array([sum(bin(int(x)).count("1") for x in r) for r in m])
        found = found or bool(np.any((bits > 1) & ((m[:, 1] | m[:, 2]) != 0)))
    assert found


def _fresh(hip, oracle, dbs, names=None, expect=SLICED, repeat=1):
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    _, _, at, dist_o, nh_o = _oracle_tables(oracle, ls, dbs)
    names = (sorted(at) if names is None else names) * repeat
    sw, info = _sweep(ls, names)
    if expect is not None:
        assert info["variant"] == expect, info
    _check(sw, names, at, dist_o, nh_o)
    return info, dist_o


def test_asymmetric_metrics(hip, oracle):
    """Metrics 1..64 drawn per direction: a relax with the wrong end's metric
    gives other distances."""
    info, dist_o = _fresh(hip, oracle, _clos400(1, 64, 8, False))
    assert info["rows"] == 400
    assert int(dist_o[dist_o != 0xFFFFFFFF].max()) == 136


def test_overloaded_nodes_and_sources(hip, oracle):
    """Overloaded FSW, spine and RSW, all of them sources too: each reaches
    its neighbours and carries no transit."""
    dbs = _clos400(1, 4, 9, False)
    for db in dbs:
        if db.thisNodeName in ("2-0-3", "1-2-5", "3-1-7"):
            db.isOverloaded = True
    _fresh(hip, oracle, dbs)


def test_u16_overflow_rows_redone(hip, oracle):
    """Metrics 19,990..20,000: every row holds a label past the u16 limit, so
    every batch flags its rows and the two-phase plan's search redoes them."""
    info, dist_o = _fresh(hip, oracle, _clos400(19_990, 20_000, 10, True))
    assert info["rows"] == 400
    assert int(dist_o[dist_o != 0xFFFFFFFF].max()) == 79_981


def test_metric_out_of_range_declines(hip, oracle):
    """One link at 40,000 (past the slot word's 15 metric bits): not the
    sliced plan, rows still right."""
    dbs = _clos400(1, 4, 7, True)
    a, b = dbs[300].thisNodeName, dbs[300].adjacencies[0].otherNodeName
    for db in dbs:
        for adj in db.adjacencies:
            if (db.thisNodeName, adj.otherNodeName) in ((a, b), (b, a)):
                adj.metric = 40_000
    info, _ = _fresh(hip, oracle, dbs, expect=None)
    assert info["variant"] != SLICED, info


def test_off_switch_keeps_two_phase_plan(clos_sym, monkeypatch):
    """ORH_WMS_SLICED=0: the per-source two-phase plan, as before the sliced
    plan existed - its rows for sources of more than 32 neighbours."""
    monkeypatch.setenv("ORH_WMS_SLICED", "0")
    c = clos_sym
    sw, info = _sweep(c["ls"], c["names"])
    assert info["variant"] in (DIST16, DIST32), info
    _check(sw, c["names"], c["at"], c["dist"], c["nh"])


def test_few_sources_decline(clos_sym):
    """100 sources (< ORH_WMS_MIN): not the sliced plan."""
    c = clos_sym
    names = random.Random(11).sample(c["names"], 100)
    sw, info = _sweep(c["ls"], names)
    assert info["variant"] != SLICED, info
    _check(sw, names, c["at"], c["dist"], c["nh"])


@pytest.mark.parametrize("env", [{}, {"ORH_WMS_SOURCES": "4"}])
@pytest.mark.parametrize("pick", ["any", "edge"])
def test_neighbour_rows_and_ragged_tail(clos_sym, monkeypatch, pick, env):
    """301 seeded sources: the neighbour rows that are no sources go to the
    scratch. 'edge' samples spines and RSWs only (at most 8 neighbours each,
    so the plan needs ORH_WMS_SLICED_ALL=1): the rows are those 301 and the
    16 FSWs, 317, a partial last batch at 8 and at 4 sources."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if pick == "edge":
        monkeypatch.setenv("ORH_WMS_SLICED_ALL", "1")
    c = clos_sym
    pool = c["names"] if pick == "any" else [n for n in c["names"] if not n.startswith("2-")]
    names = random.Random(12).sample(pool, 301)
    sw, info = _sweep(c["ls"], names)
    assert info["variant"] == SLICED and info["rows"] > 301, info
    assert info["batch_sources"] == (4 if env else 8), info
    if pick == "edge":
        assert info["rows"] == 317, info
    _check(sw, names, c["at"], c["dist"], c["nh"])


@pytest.mark.parametrize("seed", [85, 86])
def test_random_graphs_widened_envelope(hip, oracle, monkeypatch, seed):
    """Random graphs (parallel links, directional metrics, drained links and
    nodes - sources among them), every node twice as a source: the sliced
    plan under ORH_WMS_SLICED_ALL=1, the fused LDS search without it."""
    dbs = _random_weighted(seed, n=250, extra=600, max_metric=30)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    _, _, at, dist_o, nh_o = _oracle_tables(oracle, ls, dbs)
    names = sorted(at) * 2
    sw, info = _sweep(ls, names)
    assert info["variant"] == LDS_NH, info
    _check(sw, names, at, dist_o, nh_o)
    monkeypatch.setenv("ORH_WMS_SLICED_ALL", "1")
    sw, info = _sweep(ls, names)
    assert info["variant"] == SLICED and info["rows"] >= 500, info
    _check(sw, names, at, dist_o, nh_o)


def test_deltas_rebuild_the_layout(hip, oracle):
    """A metric change on an FSW adjacency, a drained link and an overloaded
    RSW after a first sweep: the next sweep's layout carries them."""
    dbs = _clos400(1, 4, 7, True)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    als_o, _, at, dist_o, nh_o = _oracle_tables(oracle, ls, dbs)
    names = sorted(at)
    sw, info = _sweep(ls, names)
    assert info["variant"] == SLICED, info
    _check(sw, names, at, dist_o, nh_o)
    by_name = {db.thisNodeName: copy.deepcopy(db) for db in dbs}
    fsw, fsw2, rsw = by_name["2-1-4"], by_name["2-0-2"], by_name["3-0-17"]
    fsw.adjacencies[40].metric = 9       # towards an RSW of its pod
    fsw2.adjacencies[5].isOverloaded = True  # a spine link, drained
    rsw.isOverloaded = True
    for db in (fsw, fsw2, rsw):
        als_h[A].update_adjacency_database(db)
        als_o[A].update_adjacency_database(db)
    order = ls.node_names()
    dist_n, nh_n = als_o[A]._impl.spf_tables(names, order, [ls.neighbors(s) for s in names], 16)
    assert not np.array_equal(dist_n, dist_o)
    sw2, info = _sweep(ls, names)
    assert info["variant"] == SLICED and info["rows"] == 400, info
    _check(sw2, names, at, dist_n, nh_n)
