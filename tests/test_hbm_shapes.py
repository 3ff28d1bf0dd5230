"""The graphs of tests/hbm_shapes.py have the properties that
test_gpu_hbm_edges.py relies on (-m "not gpu"): each is asserted from the
faithful oracle's runSpf tables (LinkState.cpp:808-882), or from the
FastChecker where named, so a shape cannot silently degenerate into one that
no longer reaches the kernel path it is there for.
"""
import random

import numpy as np
import pytest

import hbm_shapes as shapes
from openr_amd.facade import load_topology
from openr_amd.types import K_TESTING_AREA

A = K_TESTING_AREA
INF = 0xFFFFFFFF


class _Cpu:
    """A topology on the oracle, with the FastChecker's node and neighbour order."""

    def __init__(self, oracle, dbs):
        als, _ = load_topology(oracle, dbs, [])
        self.ls = als[A]._impl
        self.order = sorted(db.thisNodeName for db in dbs)
        self.at = {s: i for i, s in enumerate(self.order)}
        self.fc = oracle.module.FastChecker(self.ls, self.order)

    def nbrs(self, s):
        return [self.order[v] for v in self.fc.neighbours(self.at[s])]

    def tables(self, srcs, threads=8):
        return self.ls.spf_tables(srcs, self.order, [self.nbrs(s) for s in srcs], threads)


@pytest.fixture(scope="module")
def ring(oracle):
    dbs = shapes.two_scale_ring()
    return dbs, _Cpu(oracle, dbs)


def test_ring_mean_and_deltas(ring):
    dbs, _ = ring
    assert len(dbs) == shapes.RING_N == 613 and shapes.RING_N % 32 == 5
    assert sum(len(db.adjacencies) for db in dbs) == 1258
    assert shapes.mean_live_metric(dbs) == 1368
    assert [shapes.delta_of(dbs, p) for p in (50, 1, 100000)] == [684, 13, 1_368_000]


def test_ring_bucket_walk(ring):
    """delta 13: thirty advances of which one skips empty bucket widths (the
    way from the ring onto the chain); 684: one advance, that jump; 1,368,000:
    everything is near from the start."""
    _, g = ring
    dist, _ = g.tables(["0", "296", "612"])
    for row in dist:
        assert shapes.bucket_walk(row, 13) == (30, 1)
        assert shapes.bucket_walk(row, 684) == (1, 1)
        assert shapes.bucket_walk(row, 1_368_000) == (0, 0)


def test_bucket_walk_by_hand():
    # T = 2: 5 is 3 past it (a jump), T = 7; 8 is next (no jump), T = 10; done
    assert shapes.bucket_walk([0, 1, 5, 6, 8, 9, INF], 2) == (2, 1)
    assert shapes.bucket_walk([0, 1, 2, 3], 1) == (3, 0)
    assert shapes.bucket_walk([0], 5) == (0, 0)


def test_ring_chords_are_lowered_after_a_far_push(ring):
    """From source 0 every chord's far end is nearer round the ring than over
    the chord: the search pushes it far at the chord's weight first (the
    source is expanded before anything else) and lowers it later."""
    _, g = ring
    dist, _ = g.tables(["0"])
    for c in shapes.RING_CHORDS:
        assert dist[0][g.at[str(c)]] == min(c, 600 - c) < shapes.RING_CHORD_METRIC


@pytest.mark.parametrize("defects", [False, True])
def test_ecmp_grid_has_ecmp(oracle, defects):
    dbs = shapes.ecmp_grid(defects)
    g = _Cpu(oracle, dbs)
    srcs = ["0", "264", "528", "122"]
    dist, nh = g.tables(srcs)
    many = sum(int(np.sum(np.array([bin(int(x)).count("1") for x in nh[k][:, 0]]) >= 2)) for k in range(len(srcs)))
    print("ecmp share", many / (len(srcs) * len(g.order)))
    assert 4 * many >= len(srcs) * len(g.order)
    if defects:
        iso, ovl = g.at[str(shapes.GRID_ISOLATED)], g.at[str(shapes.GRID_OVERLOADED)]
        assert np.all(dist[:, iso] == INF) and not nh[:, iso].any()
        assert np.all(dist[:, ovl] != INF)  # reached (and no transit)
        d, m = g.tables([str(shapes.GRID_ISOLATED)])
        assert int(np.sum(d[0] != INF)) == 1 and not m[0].any()


def test_hubs_degrees_and_bit_31(oracle):
    dbs = shapes.hubs()
    assert len(dbs) == shapes.HUB_N
    a, b = str(shapes.HUB_A), str(shapes.HUB_B)
    assert len(shapes.hub_neighbours(dbs, shapes.HUB_A)) == 32
    assert len(shapes.hub_neighbours(dbs, shapes.HUB_B)) == 40
    db_a = next(d for d in dbs if d.thisNodeName == a)
    assert len(db_a.adjacencies) == 34 > 8  # parallel links: more records than ranks, a continuation at K = 4 and 8
    assert max(len(shapes.hub_neighbours(dbs, v)) for v in range(shapes.HUB_N) if v != shapes.HUB_B) == 32
    g = _Cpu(oracle, dbs)
    assert len(g.nbrs(a)) == 32 and len(g.nbrs(b)) == 40
    _, nh = g.tables([a])
    assert nh.shape[2] == 1 and (nh[0][:, 0] >> 31).any()


def _max_neighbours(dbs):
    return max(len({a.otherNodeName for a in db.adjacencies}) for db in dbs)


def _checker_equals_oracle(g, rows, seed):
    ids = random.Random(seed).sample(range(len(g.order)), rows)
    dist, nh = g.fc.spf_rows(ids, [], 8)
    od, on = g.tables([g.order[i] for i in ids])
    assert np.array_equal(dist, od)
    assert np.array_equal(nh[:, :, :1], on[:, :, :1]) and not nh[:, :, 1:].any() and not on[:, :, 1:].any()


def test_wan_small(oracle):
    dbs = shapes.wan_small()
    assert len(dbs) == 8229 and (len(dbs) + 31) // 32 == 258
    assert _max_neighbours(dbs) <= 32
    _checker_equals_oracle(_Cpu(oracle, dbs), 8, 41)


def test_wan_large(oracle):
    dbs = shapes.wan_large()
    assert len(dbs) == 32805 and (len(dbs) + 31) // 32 == 1026
    assert _max_neighbours(dbs) <= 32
    _checker_equals_oracle(_Cpu(oracle, dbs), 2, 42)


def test_tiny_and_drain_grid(oracle):
    dbs = shapes.tiny()
    assert len(dbs) == 20
    assert sum(len(db.adjacencies) for db in dbs) == 2 * 31
    g = _Cpu(oracle, dbs)
    dist, _ = g.tables(g.order)
    assert np.all(dist != INF)  # connected
    grid = shapes.drain_grid()
    assert len(grid) == 3600 and shapes.mean_live_metric(grid) == 1 and shapes.delta_of(grid) == 1
