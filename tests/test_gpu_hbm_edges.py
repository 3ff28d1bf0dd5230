"""The HBM frontier searches at their word and bucket edges (``-m gpu``):
spf_global_kernel (ORH_VARIANT_GLOBAL, two-phase: the generic first-hop kernel
over its u32 rows) and spf_global_nh_async_kernel (ORH_VARIANT_GLOBAL_NH, first
hops fused, asynchronous buckets) through its sweep, ignore-set and what-if
full-search callers. Every compared row - dist and every first-hop mask word -
is bit for bit the faithful oracle's runSpf table (LinkState.cpp:808-882), or
the FastChecker's where a sweep has more rows than the oracle can do in
seconds; the plan (variant, rows) comes from orh_last_spf_info.

The graphs are those of tests/hbm_shapes.py, whose properties (bucket counts,
ECMP share, hub ranks, NB) tests/test_hbm_shapes.py pins on the CPU:

  a  ring 613     mode 2  all 613        256 threads over 20 words, the partial
                                         last word, chords pushed far and
                                         lowered into the near set, one
                                         threshold jump
  b  ring 613     mode 2  40 + 3         1,024 threads over 20 words: most waves
                                         idle from the start, leave on s_work
  c  ring 613     mode 3  6              spf_global_kernel, neighbour rows in
                                         scratch
  d  ecmp grid    2, 3    all            equal-distance merges that re-queue; an
     (+ defects)                         overloaded node, a drained link, INF rows
  e  hubs         mode 2  53, never B    one mask word, bit 31, rank_out of the
                                         overflow records, parallel links
  f  hubs         mode 2  the same + B   40 neighbours: GLOBAL even in mode 2,
                                         two mask words
  g  wan 8,229    mode 3  8              spf_global_kernel, 256 threads over 258
                                         words: threads 0 and 1 own two
  h  wan 8,229    mode 2  520            GLOBAL_NH, 256 threads over 258 words:
                                         the rescan wraps to a second word
  i  wan 32,805   mode 2  6              1,024 threads over 1,026 words
  j  wan 8,229    auto    8, then 40     the LDS kernels on the same graph

then the bucket width (ORH_DELTA_PCT, read at orh_create: a child process per
value), ignore sets through the hashed LDS filter at FW = 1, 16 and 256, hop
counts (delta = 1), and the what-if job's full search (row_list / row_count,
the kDrain instantiation) on general metrics. The job's row_mask fallback
(n_slots == 0) needs a graph so large that not one repair slot fits the 1 GB
slot budget; no knob reaches it, so it is not run here.
"""
import dataclasses
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import hbm_shapes as shapes
from openr_amd import host_module
from openr_amd.facade import load_topology
from openr_amd.types import K_TESTING_AREA
from test_gpu_weighted import _compare_rows
from test_gpu_whatif_drain import Oracles, _check_rows, _run

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = 0xFFFFFFFF
DIST32, GLOBAL, GLOBAL_NH, LDS_NH = 6, 7, 8, 12  # ORH_VARIANT_*
AUTO, GLOBAL_MODE, GLOBAL_TWO_PHASE = 0, 2, 3     # orh_set_spf_mode


def _plan(sw, variant, rows, label):
    info = sw.info()
    print("plan", label, int(info["variant"]), int(info["rows"]))
    assert (int(info["variant"]), int(info["rows"])) == (variant, rows), (label, info)


def _sweep(ls, names, mode, variant, rows, label):
    mod = host_module()
    mod.set_spf_mode(mode)
    try:
        sw = ls.sweep(names, True)
        sw.run()
        sw.sync()
        _plan(sw, variant, rows, label)
    finally:
        mod.set_spf_mode(0)
    return sw


def _two_phase_rows(ls, names):
    return len(set(names) | {u for s in names for u in ls.neighbors(s)})


class _Small:
    """A graph the oracle searches from every node in well under a second:
    the tables of all nodes as sources, read-only."""

    def __init__(self, hip, oracle, dbs):
        self.dbs = dbs
        self.als, _ = load_topology(hip, dbs, [])
        self.ls = self.als[A]._impl
        self.als_o, _ = load_topology(oracle, dbs, [])
        self.names = sorted(db.thisNodeName for db in dbs)
        self.order = self.ls.node_names()
        self.dist, self.nh = self.als_o[A]._impl.spf_tables(
            self.names, self.order, [self.ls.neighbors(s) for s in self.names], 16)
        self.dist.setflags(write=False)
        self.nh.setflags(write=False)
        self.at = {s: k for k, s in enumerate(self.names)}

    def want(self, names):
        idx = [self.at[s] for s in names]
        return self.dist[idx], self.nh[idx]

    def sweep(self, names, mode, variant, rows, label):
        sw = _sweep(self.ls, names, mode, variant, rows, label)
        _compare_rows(sw, names, list(range(len(names))), *self.want(names), label)
        return sw

    def ignore_tables(self, srcs, sets, desc, ls_o=None):
        return (ls_o or self.als_o[A]._impl).spf_tables(
            srcs, self.order, [self.ls.neighbors(s) for s in srcs], 16,
            [[tuple(desc[l][:3]) for l in st] for st in sets])


class _Wan:
    """A WAN on the HIP backend, the oracle and the FastChecker (in the
    product's node order, so ids and first-hop ranks are the device's)."""

    def __init__(self, hip, oracle, dbs):
        self.dbs = dbs
        self.als, _ = load_topology(hip, dbs, [])
        self.ls = self.als[A]._impl
        self.als_o, _ = load_topology(oracle, dbs, [])
        self.order = self.ls.node_names()
        self.ids = {s: i for i, s in enumerate(self.order)}
        self.fc = oracle.module.FastChecker(self.als_o[A]._impl, self.order)

    def check(self, sw, names, oracle_rows, label):
        """Every row against the FastChecker, rows ``oracle_rows`` against the
        faithful oracle too."""
        dist, nh = self.fc.spf_rows([self.ids[s] for s in names], [], 16)
        _compare_rows(sw, names, list(range(len(names))), dist, nh, label + " checker")
        srcs = [names[i] for i in oracle_rows]
        dist_o, nh_o = self.als_o[A]._impl.spf_tables(srcs, self.order, [self.ls.neighbors(s) for s in srcs], 16)
        _compare_rows(sw, names, oracle_rows, dist_o, nh_o, label + " oracle")
        return dist


@pytest.fixture(scope="module")
def ring(hip, oracle):
    return _Small(hip, oracle, shapes.two_scale_ring())


@pytest.fixture(scope="module")
def grid(hip, oracle):
    return _Small(hip, oracle, shapes.ecmp_grid())


@pytest.fixture(scope="module")
def hubs(hip, oracle):
    return _Small(hip, oracle, shapes.hubs())


@pytest.fixture(scope="module")
def tiny(hip, oracle):
    return _Small(hip, oracle, shapes.tiny())


@pytest.fixture(scope="module")
def wan_small(hip, oracle):
    return _Wan(hip, oracle, shapes.wan_small())


# ---- sweeps -----------------------------------------------------------------

def test_a_ring_all_sources_global_nh(ring):
    """613 sources, more than two per CU: 256 threads. At the product's
    delta of 684 every chord end is pushed far at 50,000 from source 0 and
    lowered into the near set of the first bucket; one threshold jump takes
    the search onto the chain."""
    g = ring
    assert shapes.delta_of(g.dbs) == 684
    for s in ("0", "296", "612"):
        assert shapes.bucket_walk(g.dist[g.at[s]], 684) == (1, 1)
    g.sweep(g.names, GLOBAL_MODE, GLOBAL_NH, 613, "a ring all")


def test_b_ring_few_sources_1024_threads(ring):
    """43 sources, at most one per CU: 1,024 threads over 20 bitmap words, so
    15 of 16 waves never own a word and leave on the work count alone."""
    g = ring
    names = shapes.ring_few_sources()
    assert len(set(names)) == 43
    g.sweep(names, GLOBAL_MODE, GLOBAL_NH, 43, "b ring 43")


def test_c_ring_two_phase_global(ring):
    g = ring
    names = shapes.RING_TWO_PHASE_SOURCES
    rows = _two_phase_rows(g.ls, names)
    assert rows > len(names)  # neighbour rows in scratch
    g.sweep(names, GLOBAL_TWO_PHASE, GLOBAL, rows, "c ring two-phase")


@pytest.mark.parametrize("mode,variant", [(GLOBAL_MODE, GLOBAL_NH), (GLOBAL_TWO_PHASE, GLOBAL)])
def test_d_ecmp_grid(grid, mode, variant):
    g = grid
    ecmp = np.array([[bin(int(x)).count("1") for x in g.nh[k][:, 0]] for k in range(0, len(g.names), 23)])
    assert 4 * int(np.sum(ecmp >= 2)) >= ecmp.size
    g.sweep(g.names, mode, variant, len(g.names), f"d grid mode {mode}")


@pytest.mark.parametrize("mode,variant", [(GLOBAL_MODE, GLOBAL_NH), (GLOBAL_TWO_PHASE, GLOBAL)])
def test_d_ecmp_grid_defects(hip, oracle, mode, variant):
    """An overloaded interior node (reached, no transit; a source like any
    other), a drained link, and an isolated node: INF in every other row with
    zero masks, and a row of its own that reaches nothing."""
    g = _Small(hip, oracle, shapes.ecmp_grid(defects=True))
    iso, iso_row = g.order.index(str(shapes.GRID_ISOLATED)), g.at[str(shapes.GRID_ISOLATED)]
    assert np.all(np.delete(g.dist[:, iso], iso_row) == INF)
    assert np.all(np.delete(g.dist[:, g.order.index(str(shapes.GRID_OVERLOADED))], iso_row) != INF)
    assert int(np.sum(g.dist[iso_row] != INF)) == 1 and not g.nh[iso_row].any()
    g.sweep(g.names, mode, variant, len(g.names), f"d grid defects mode {mode}")


def _hub_sources(g):
    a, b = str(shapes.HUB_A), str(shapes.HUB_B)
    nbrs = g.ls.neighbors(a)
    assert len(nbrs) == 32 and len(g.ls.neighbors(b)) == 40
    rest = [s for s in g.names if s not in set(nbrs) | {a, b}]
    return [a] + nbrs + random.Random(3101).sample(rest, 20)


def test_e_hubs_bit_31(hubs):
    """Hub A's 32 neighbours fill the one mask word; its 34 records (parallel
    links) continue in the overflow area, where rank_out is read per record."""
    g = hubs
    names = _hub_sources(g)
    assert (g.nh[g.at[str(shapes.HUB_A)]][:, 0] >> 31).any()
    assert max(len(g.ls.neighbors(s)) for s in names) == 32
    sw = g.sweep(names, GLOBAL_MODE, GLOBAL_NH, len(names), "e hubs without B")
    assert sw.words == 1


def test_f_hubs_two_words_stay_two_phase(hubs):
    """With hub B (40 neighbours) among the sources the fused kernel does not
    apply: spf_global_kernel even in mode 2, two mask words."""
    g = hubs
    names = _hub_sources(g) + [str(shapes.HUB_B)]
    sw = g.sweep(names, GLOBAL_MODE, GLOBAL, _two_phase_rows(g.ls, names), "f hubs with B")
    assert sw.words == 2
    assert g.nh[g.at[str(shapes.HUB_B)]][:, 1].any()


def _wan_eight(g):
    return random.Random(3300).sample(g.order, 8)


def test_g_wan_two_phase_258_words(wan_small):
    g = wan_small
    names = _wan_eight(g)
    sw = _sweep(g.ls, names, GLOBAL_TWO_PHASE, GLOBAL, _two_phase_rows(g.ls, names), "g wan 8229 mode 3")
    g.check(sw, names, list(range(8)), "g")


def test_h_wan_rescan_wrap(wan_small):
    """520 sources, more than two per CU: 256 threads over 258 words, so
    threads 0 and 1 come back to a second word of their own."""
    g = wan_small
    names = random.Random(3301).sample(g.order, 520)
    sw = _sweep(g.ls, names, GLOBAL_MODE, GLOBAL_NH, 520, "h wan 8229 mode 2")
    g.check(sw, names, list(range(0, 520, 65)), "h")


def test_i_wan_1026_words(hip, oracle):
    """6 sources: 1,024 threads over 1,026 words. The sources are the device
    ids at the ends of the first, a middle and the last bitmap word and
    either side of 2^15."""
    g = _Wan(hip, oracle, shapes.wan_large())
    assert len(g.order) == shapes.WAN_LARGE
    names = [g.order[i] for i in (0, 31, 32, 32767, 32768, 32804)]
    sw = _sweep(g.ls, names, GLOBAL_MODE, GLOBAL_NH, 6, "i wan 32805 mode 2")
    g.check(sw, names, [1, 5], "i")


def test_j_wan_lds_kernels_agree(wan_small):
    """The same graph through the plans the product picks on its own: 8
    sources are below ORH_LDS_NH_MIN (two-phase, u32 labels: the path bound is
    past 16 bits), 40 take the fused LDS search."""
    g = wan_small
    names = _wan_eight(g)
    sw = _sweep(g.ls, names, AUTO, DIST32, _two_phase_rows(g.ls, names), "j wan 8229 auto 8")
    g.check(sw, names, list(range(8)), "j 8")
    names = random.Random(3302).sample(g.order, 40)
    sw = _sweep(g.ls, names, AUTO, LDS_NH, 40, "j wan 8229 auto 40")
    g.check(sw, names, [0, 39], "j 40")


# ---- bucket widths ----------------------------------------------------------

_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
import hbm_shapes as shapes
from openr_amd import host_backend, host_module
from openr_amd.facade import load_topology
from openr_amd.types import K_TESTING_AREA as A
out = {}


def case(tag, dbs, names, mode):
    als, _ = load_topology(host_backend(), dbs, [])
    ls = als[A]._impl
    host_module().set_spf_mode(mode)
    try:
        sw = ls.sweep(names, True)
        sw.run()
        sw.sync()
        info = sw.info()
    finally:
        host_module().set_spf_mode(0)
    rows = [sw.fetch(i) for i in range(len(names))]
    out[tag + "_dist"] = np.stack([r[0] for r in rows])
    out[tag + "_nh"] = np.stack([r[1] for r in rows])
    out[tag + "_plan"] = np.array([int(info["variant"]), int(info["rows"])])


ring = shapes.two_scale_ring()
case("a", ring, shapes.ring_few_sources(), 2)
case("c", ring, shapes.RING_TWO_PHASE_SOURCES, 3)
grid = shapes.ecmp_grid()
case("d", grid, sorted(db.thisNodeName for db in grid), 2)
np.savez(sys.argv[2], **out)
"""


@pytest.mark.parametrize("pct", ["1", "100000"])
def test_bucket_widths(ring, grid, tmp_path, pct):
    """ORH_DELTA_PCT = 1: delta 13 on the ring (30 threshold advances per
    search, one of them a jump) and 1 on the grid (a bucket per distance);
    100000: delta 1,368,000 and 1,000, every node near from the start, so the
    whole search is one asynchronous bucket. Same rows either way."""
    delta = shapes.delta_of(ring.dbs, int(pct))
    assert delta == {"1": 13, "100000": 1_368_000}[pct]
    assert shapes.bucket_walk(ring.dist[ring.at["0"]], delta) == {"1": (30, 1), "100000": (0, 0)}[pct]
    assert shapes.delta_of(grid.dbs, int(pct)) == {"1": 1, "100000": 1000}[pct]
    out = tmp_path / "rows.npz"
    env = dict(os.environ, ORH_DELTA_PCT=pct)
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out)], check=True, env=env, timeout=120)
    got = np.load(out)
    few, six = shapes.ring_few_sources(), shapes.RING_TWO_PHASE_SOURCES
    for tag, g, names, plan in (("a", ring, few, (GLOBAL_NH, 43)),
                                ("c", ring, six, (GLOBAL, _two_phase_rows(ring.ls, six))),
                                ("d", grid, grid.names, (GLOBAL_NH, len(grid.names)))):
        print("plan", tag, pct, got[tag + "_plan"])
        assert tuple(int(x) for x in got[tag + "_plan"]) == plan, (tag, pct)
        dist, nh = g.want(names)
        assert np.array_equal(got[tag + "_dist"], dist), (tag, pct)
        m = got[tag + "_nh"].reshape(len(names), len(g.order), -1)
        w = min(m.shape[2], nh.shape[2])
        assert np.array_equal(m[:, :, :w], nh[:, :, :w]), (tag, pct)
        assert not m[:, :, w:].any() and not nh[:, :, w:].any()


# ---- ignore sets ------------------------------------------------------------

def _ignore_batch(ls, srcs, seed, big):
    """Per source: one link, three links, every link of the source's first
    neighbour plus seeded links up to ``big``, and no link at all."""
    rng = random.Random(seed)
    desc = dict(ls.link_ids())
    lids = sorted(desc)
    out_srcs, sets = [], []
    for s in srcs:
        first = ls.neighbors(s)[0]
        large = [l for l in lids if first in (desc[l][0], desc[l][2])]
        taken = set(large)
        pool = [l for l in lids if l not in taken]
        large = large + rng.sample(pool, max(0, big - len(large)))
        for st in ([rng.choice(lids)], rng.sample(lids, 3), large, []):
            out_srcs.append(s)
            sets.append(st)
    return out_srcs, sets, desc


def _ignore_sweep(ls, srcs, sets, mode, variant, label, use_link_metric=True):
    mod = host_module()
    mod.set_spf_mode(mode)
    try:
        sw = ls.what_if_sweep(srcs, sets, use_link_metric)
        sw.run()
        sw.sync()
        info = sw.info()
    finally:
        mod.set_spf_mode(0)
    print("plan", label, int(info["variant"]), int(info["rows"]))
    assert int(info["variant"]) == variant, (label, info)
    # fused: a row per request; two-phase: the neighbours' rows under the same set too
    assert int(info["rows"]) == len(srcs) if variant == GLOBAL_NH else int(info["rows"]) > len(srcs), (label, info)
    return sw


@pytest.mark.parametrize("mode,variant", [(GLOBAL_MODE, GLOBAL_NH), (GLOBAL_TWO_PHASE, GLOBAL)])
def test_ignore_sets_tiny_one_word_filter(tiny, mode, variant):
    """NB = 1, FW = 1: a 32-bit filter that twelve links fill, so nearly every
    record goes on to the binary search. All 20 sources."""
    g = tiny
    srcs, sets, desc = _ignore_batch(g.ls, g.names, 3400, 12)
    assert max(len(st) for st in sets) == 12
    sw = _ignore_sweep(g.ls, srcs, sets, mode, variant, f"ignore tiny mode {mode}")
    dist, nh = g.ignore_tables(srcs, sets, desc)
    assert np.any(dist == INF)  # a first neighbour cut off
    _compare_rows(sw, srcs, list(range(len(srcs))), dist, nh, f"ignore tiny mode {mode}")


@pytest.mark.parametrize("mode,variant", [(GLOBAL_MODE, GLOBAL_NH), (GLOBAL_TWO_PHASE, GLOBAL)])
def test_ignore_sets_ring(ring, mode, variant):
    """NB = 20: FW = 16. Source 0's first neighbour loses every link; the
    chords and the spur are in reach of the seeded picks."""
    g = ring
    srcs, sets, desc = _ignore_batch(g.ls, shapes.RING_TWO_PHASE_SOURCES + ["150", "450", "606"], 3401, 64)
    assert max(len(st) for st in sets) == 64
    sw = _ignore_sweep(g.ls, srcs, sets, mode, variant, f"ignore ring mode {mode}")
    dist, nh = g.ignore_tables(srcs, sets, desc)
    _compare_rows(sw, srcs, list(range(len(srcs))), dist, nh, f"ignore ring mode {mode}")


def test_ignore_sets_ring_hop_counts(ring, oracle):
    """use_link_metric = False: every link counts 1, the search is uniform
    and delta = 1, a bucket per BFS level. The reference is the oracle on the
    same graph with every metric set to 1."""
    g = ring
    srcs, sets, desc = _ignore_batch(g.ls, shapes.RING_TWO_PHASE_SOURCES, 3402, 64)
    sw = _ignore_sweep(g.ls, srcs, sets, GLOBAL_MODE, GLOBAL_NH, "ignore ring hops", use_link_metric=False)
    unit = [dataclasses.replace(db, adjacencies=[dataclasses.replace(a, metric=1) for a in db.adjacencies])
            for db in g.dbs]
    als_u, _ = load_topology(oracle, unit, [])
    dist, nh = g.ignore_tables(srcs, sets, desc, als_u[A]._impl)
    assert int(dist[dist != INF].max()) < 400  # hops, not metrics
    _compare_rows(sw, srcs, list(range(len(srcs))), dist, nh, "ignore ring hops")


def test_ignore_sets_wan_filter_cap(wan_small):
    """NB = 258: FW = 256, the filter's cap."""
    g = wan_small
    srcs, sets, desc = _ignore_batch(g.ls, random.Random(3403).sample(g.order, 3), 3404, 64)
    sw = _ignore_sweep(g.ls, srcs, sets, GLOBAL_MODE, GLOBAL_NH, "ignore wan 8229")
    dist, nh = g.als_o[A]._impl.spf_tables(srcs, g.order, [g.ls.neighbors(s) for s in srcs], 16,
                                           [[tuple(desc[l][:3]) for l in st] for st in sets])
    _compare_rows(sw, srcs, list(range(len(srcs))), dist, nh, "ignore wan 8229")


# ---- the what-if job's full search -------------------------------------------

def test_whatif_full_search_weighted(hip, oracle):
    """test_drain_tiers' 60 x 60 layout with horizontal links at 1 and
    vertical ones at 2 (general metrics, delta = 1). With search_large the
    requests past tier 1 are searched in full by spf_global_nh_async_kernel
    over the job's row list, drains and ignore sets included; the same job
    without the flag repairs them and must give the same rows."""
    dbs = shapes.drain_grid()
    assert shapes.delta_of(dbs) == 1
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    desc = dict(ls.link_ids())

    def link(a, b):
        (lid,) = [l for l, d in desc.items() if {d[0], d[2]} == {a, b}]
        return lid

    srcs = ["0", "1830"]
    far = ["3599", "3598", "3539", "3478", "3300"]
    reqs = [(0, "1", ())] * 35 + [(1, "1831", ())] + [(0, x, ()) for x in far] + [(0, "1", ())] * 35
    # a drain and an ignored link: 0 cut down to its drained neighbour (all but
    # 0 and 1 unreached), a link behind the drained node, two round 1830
    reqs += [(0, "1", (link("0", "60"),)), (0, "1", (link("61", "62"),)),
             (1, "1831", (link("1830", "1770"),)), (1, "1831", (link("1830", "1890"),))]
    idx = [k for k, _, _ in reqs]
    drain = [[x] for _, x, _ in reqs]
    ignore = [list(l) for _, _, l in reqs]
    full = _run(ls, srcs, idx, ignore, drain, search_large=True)
    tier = full.info() & 7
    print("tiers", sorted(set(int(t) for t in tier)), "searched in full:", int(np.sum(tier == 4)))
    assert np.any(tier == 4)
    first = {}
    for i, r in enumerate(reqs):
        first.setdefault(r, i)
    assert len(first) == 11
    _check_rows(ls, full, Oracles(oracle, dbs), srcs, idx, ignore, drain, desc, which=sorted(first.values()))
    rows = [full.fetch(i) for i in range(len(reqs))]
    for i, r in enumerate(reqs):
        t = first[r]
        assert np.array_equal(rows[i][0], rows[t][0]) and np.array_equal(rows[i][1], rows[t][1]), (i, r)
    cut = rows[first[reqs[76]]][0]
    assert int(np.sum(cut != INF)) == 2
    del full
    plain = _run(ls, srcs, idx, ignore, drain)
    assert not np.any((plain.info() & 7) == 4)
    for i in range(len(reqs)):
        d, m = plain.fetch(i)
        assert np.array_equal(d, rows[i][0]) and np.array_equal(m, rows[i][1]), (i, reqs[i])
