"""Weighted all-sources sweeps whose metrics pass the 15 bits of the u16
plans' slot word: the wide multi-source Bellman-Ford plan (spf_wms_wide_kernel,
ORH_VARIANT_WMS_WIDE: u32 labels, full u32 metrics, 4 or 2 sources per batch),
which takes exactly the sweeps the WMS and sliced WMS plans decline for their
metric range alone, and the wide redo of the rows those two plans flag. Every
checked row - dist and every first-hop mask word - against the faithful
oracle's runSpf tables (LinkState.cpp:808-882). Shape properties (metrics and
distances past 16 bits, ECMP past rank 31) are asserted from the oracle's
tables, not as constants.

  clos400   fabric(400, bug_compatible=False): 288 spines of degree 2, 16 FSWs
            of degree 84, 96 RSWs of degree 8; 3 mask words; seeded metrics
            30,000..70,000
  ring300   test_gpu_spf_plan_table._low_degree_300 at 5,000 times its metrics
            (every degree <= 8: the WMS plan's shape)
  random    test_gpu_parity.random_topology graphs (degree <= 32) at metrics up
            to 60,000
"""
import copy
import random

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import ladder
from openr_amd.types import K_TESTING_AREA
from test_gpu_spf_plan_table import _low_degree_300
from test_gpu_weighted import _random_weighted
from test_gpu_weighted_sliced import _check, _clos400, _oracle_tables, _sweep

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
DIST16, DIST32, EXACT, LDS_NH, WMS, SLICED, WIDE = 5, 6, 9, 12, 13, 14, 15  # ORH_VARIANT_*
INF = 0xFFFFFFFF
KNOBS = ("ORH_WMS_WIDE", "ORH_WMS_WIDE_SOURCES", "ORH_WMS_WIDE_REDO", "ORH_WMS_SLICED", "ORH_WMS_SLICED_ALL",
         "ORH_WMS_SLICED_BLOCK", "ORH_WMS_SOURCES")


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _max_metric(dbs):
    return max(adj.metric for db in dbs for adj in db.adjacencies)


def _loaded(hip, oracle, dbs):
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    als_o, _, at, dist_o, nh_o = _oracle_tables(oracle, ls, dbs)
    dist_o.setflags(write=False)
    nh_o.setflags(write=False)
    return {"dbs": dbs, "als": als_h, "als_o": als_o, "ls": ls, "names": sorted(at), "at": at, "dist": dist_o,
            "nh": nh_o}


def _run(c, names=None, expect=WIDE):
    names = c["names"] if names is None else names
    sw, info = _sweep(c["ls"], names)
    if expect is not None:
        assert info["variant"] == expect, info
    _check(sw, names, c["at"], c["dist"], c["nh"])
    return sw, info


def _clos400_coarse(seed):
    """Symmetric metrics 30,000..70,000 in steps of 10,000: equal-cost paths
    are common, as they are at metrics 1..4 (uniform draws over the whole
    range leave next to none)."""
    dbs = _clos400(3, 7, seed, True)
    for db in dbs:
        for adj in db.adjacencies:
            adj.metric *= 10_000
    return dbs


@pytest.fixture(scope="module")
def clos_wide(hip, oracle):
    """Case 1's graph (symmetric metrics 30,000..70,000, seed 7) on both
    backends and the oracle's tables of all 400 sources, shared by the tests
    that sweep it."""
    return _loaded(hip, oracle, _clos400_coarse(7))


def test_clos_all_sources_wide(clos_wide):
    """All 400 sources: the wide plan (the per-source two-phase plan before),
    4 sources per batch, then every first hop from the u32 rows. Slot metrics
    past 15 bits, distances past 16 bits, 3 mask words, ECMP sets that reach
    past rank 31."""
    c = clos_wide
    sw, info = _run(c)
    assert info["variant"] == WIDE and info["rows"] == 400 and info["batch_sources"] == 4, info
    assert info["hop_nodes"] == 1 and info["wide_redo"] == 0, info
    assert info["ms_threads"] in (256, 512, 1024) and info["wsl_slots"] >= info["wsl_links"] > 0, info
    assert _max_metric(c["dbs"]) > 0x7FFF
    finite = c["dist"][c["dist"] != INF]
    # RSW to RSW of another pod: >= 4 links of >= 30,000 each, past 16 bits
    assert int(finite.max()) >= 120_000 > 0xFFFF
    assert sw.words == 3
    nh = c["nh"]  # [source][node][word]: some ECMP set holds a neighbour of rank >= 32
    several = (nh & (nh - 1)).any(axis=2) | ((nh != 0).sum(axis=2) > 1)
    assert bool(np.any(several & (nh[:, :, 1:] != 0).any(axis=2)))


def test_asymmetric_metrics(hip, oracle):
    """Metrics 30,000..70,000 drawn per direction: a relax with the wrong
    end's metric gives other distances."""
    dbs = _clos400(30_000, 70_000, 8, False)
    metric = {(db.thisNodeName, adj.otherNodeName): adj.metric for db in dbs for adj in db.adjacencies}
    assert any(w != metric[(b, a)] for (a, b), w in metric.items())
    c = _loaded(hip, oracle, dbs)
    _, info = _run(c)
    assert info["rows"] == 400 and info["batch_sources"] == 4, info


@pytest.mark.parametrize("sources", [2, 4])
@pytest.mark.parametrize("pick", ["any", "edge"])
def test_neighbour_rows_and_ragged_tail(clos_wide, monkeypatch, pick, sources):
    """301 seeded sources: the neighbour rows that are no sources go to the
    scratch. 'edge' samples spines and RSWs only (at most 8 neighbours each,
    so the plan needs ORH_WMS_SLICED_ALL=1): the rows are those 301 and the
    FSWs, an odd count, so the last batch is partial at 2 and at 4 sources.
    ORH_WMS_WIDE_SOURCES=2: the 2-source instantiation."""
    if sources == 2:
        monkeypatch.setenv("ORH_WMS_WIDE_SOURCES", "2")
    if pick == "edge":
        monkeypatch.setenv("ORH_WMS_SLICED_ALL", "1")
    c = clos_wide
    pool = c["names"] if pick == "any" else [n for n in c["names"] if not n.startswith("2-")]
    names = random.Random(12).sample(pool, 301)
    rows = len(set(names) | {u for s in names for u in c["ls"].neighbors(s)})
    assert rows > 301 and (pick == "any" or rows % 2 == 1)
    _, info = _run(c, names)
    assert info["rows"] == rows and info["batch_sources"] == sources, info


def test_overloaded_nodes_sources_and_drained_link(hip, oracle):
    """Overloaded FSW, spine and RSW, all of them sources too, and a drained
    link: the pass before the rounds, dead slots, sources that reach their
    neighbours only."""
    dbs = _clos400(30_000, 70_000, 9, False)
    ovl = ("2-0-3", "1-2-5", "3-1-7")
    for db in dbs:
        if db.thisNodeName in ovl:
            db.isOverloaded = True
        if db.thisNodeName == "2-1-4":
            db.adjacencies[7].isOverloaded = True
    c = _loaded(hip, oracle, dbs)
    _run(c)
    # an overloaded source reaches its neighbours; nothing transits it
    row = c["dist"][c["at"]["3-1-7"]]
    assert int((row != INF).sum()) > 1


def test_low_degree_graph_takes_wide_by_default(hip, oracle, monkeypatch):
    """Every degree <= 8 (the WMS plan's shape) at 5,000 times the metrics:
    the wide plan by default; ORH_WMS_WIDE=0: the fused LDS search, as before,
    and the same rows."""
    dbs = _low_degree_300()
    for db in dbs:
        for adj in db.adjacencies:
            adj.metric *= 5000
    assert _max_metric(dbs) > 0x7FFF
    c = _loaded(hip, oracle, dbs)
    _, info = _run(c)
    assert info["rows"] == 300 and info["batch_sources"] == 4, info
    monkeypatch.setenv("ORH_WMS_WIDE", "0")
    _run(c, expect=LDS_NH)


@pytest.mark.parametrize("seed", [85, 86])
def test_random_graphs_need_the_opt_in(hip, oracle, monkeypatch, seed):
    """Random graphs (parallel links, directional metrics up to 60,000,
    drained links and nodes, isolated nodes - sources among them), every node
    twice as a source: sources of <= 32 neighbours keep the fused LDS search;
    under ORH_WMS_SLICED_ALL=1 the wide plan, repeated sources inside a batch."""
    dbs = _random_weighted(seed, n=250, extra=600, max_metric=60_000)
    assert _max_metric(dbs) > 0x7FFF
    c = _loaded(hip, oracle, dbs)
    names = c["names"] * 2
    _run(c, names, expect=LDS_NH)
    monkeypatch.setenv("ORH_WMS_SLICED_ALL", "1")
    _, info = _run(c, names)
    assert info["rows"] >= 500, info


def test_few_sources_decline(clos_wide):
    """100 sources (< ORH_WMS_MIN): not the wide plan."""
    c = clos_wide
    names = random.Random(11).sample(c["names"], 100)
    _, info = _run(c, names, expect=None)
    assert info["variant"] != WIDE, info


def test_wide_path_metrics_go_to_the_exact_kernel(hip, oracle):
    """One link at 2^31 - 1, the largest metric an adjacency carries (the field
    is an i32 on the wire, so 3,000,000,000 cannot be loaded): the sum of the
    metrics plus the largest passes 2^32 - 1, so a path sum may reach the
    unreached value, which the wide kernel's saturating add does not cover.
    A sweep into u32 rows is refused, as before the wide plan (it names the
    exact entry point); the searches LinkState runs itself go to the exact
    kernel, and their results are the oracle's."""
    dbs = _clos400_coarse(7)
    a, b = dbs[300].thisNodeName, dbs[300].adjacencies[0].otherNodeName
    for db in dbs:
        for adj in db.adjacencies:
            if (db.thisNodeName, adj.otherNodeName) in ((a, b), (b, a)):
                adj.metric = 0x7FFFFFFF
    total = sum(adj.metric for db in dbs for adj in db.adjacencies) // 2
    assert total + 0x7FFFFFFF >= 0xFFFFFFFF
    als_h, _ = load_topology(hip, dbs, [])
    als_o, _ = load_topology(oracle, dbs, [])
    ls = als_h[A]._impl
    names = sorted(db.thisNodeName for db in dbs)
    with pytest.raises(RuntimeError, match="orh_spf_run_exact"):
        _sweep(ls, names)
    for src in (a, b, "2-0-3", "3-1-7"):
        got, want = (als[A].get_spf_result(src) for als in (als_h, als_o))
        assert ls.last_spf_info()["variant"] == EXACT
        assert {k: (v.metric, v.nextHops) for k, v in got.items()} == \
               {k: (v.metric, v.nextHops) for k, v in want.items()}, src


def test_deltas_move_the_sweep_between_layouts(hip, oracle):
    """Metrics 1..4: the sliced plan. One FSW adjacency at 50,000: the wide
    plan. Back to 3: the sliced plan again. The rows are right each time."""
    c = _loaded(hip, oracle, _clos400(1, 4, 7, True))
    names, ls = c["names"], c["ls"]
    _run(c, expect=SLICED)
    fsw = copy.deepcopy(next(db for db in c["dbs"] if db.thisNodeName == "2-1-4"))
    nbrs = [ls.neighbors(s) for s in names]
    # an adjacency at metric 1 towards an RSW: the FSW's shortest path to it, so either change shows
    k = next(i for i, adj in enumerate(fsw.adjacencies) if adj.metric == 1 and adj.otherNodeName.startswith("3-"))
    for metric, want in ((50_000, WIDE), (3, SLICED)):
        fsw.adjacencies[k].metric = metric
        for als in (c["als"], c["als_o"]):
            als[A].update_adjacency_database(copy.deepcopy(fsw))
        dist_n, nh_n = c["als_o"][A]._impl.spf_tables(names, ls.node_names(), nbrs, 16)
        assert not np.array_equal(dist_n, c["dist"])
        sw, info = _sweep(ls, names)
        assert info["variant"] == want and info["rows"] == 400, (metric, info)
        _check(sw, names, c["at"], dist_n, nh_n)


def _ladder_20k():
    dbs, _ = ladder(130, metric=20_000)
    for db in dbs[::5]:
        db.adjacencies[0].metric = 19_999
    return dbs


@pytest.mark.parametrize("graph,variant,repeat", [("clos", SLICED, 1), ("ladder", WMS, 2)])
def test_flagged_rows_redone_in_wide_batches(hip, oracle, monkeypatch, graph, variant, repeat):
    """Metrics near 20,000 fit the u16 plans' slots, the distances do not fit
    their labels: every batch flags its rows. By default the wide kernel's
    row-list entry redoes them in batches (info wide_redo: its batch width);
    ORH_WMS_WIDE_REDO=0: per source, as before. The same plan and rows."""
    dbs = _clos400(19_990, 20_000, 10, True) if graph == "clos" else _ladder_20k()
    assert _max_metric(dbs) <= 0x7FFF
    c = _loaded(hip, oracle, dbs)
    # every row holds a finite distance past the u16 labels
    assert all(int(r[r != INF].max()) > 0xFFFF for r in c["dist"])
    names = c["names"] * repeat
    _, info = _run(c, names, expect=variant)
    assert info["wide_redo"] == 4, info
    monkeypatch.setenv("ORH_WMS_WIDE_REDO", "0")
    _, info = _run(c, names, expect=variant)
    assert info["wide_redo"] == 0, info
