"""Node-drain requests of what-if jobs (orh_whatif_run_drains) against the
oracle (``-m gpu``).

A request may name nodes to be treated as overloaded ("what if I drain this
node?", LinkState::updateNodeOverloaded, LinkState.cpp:480-493): the node stays
reachable and carries no transit traffic (:831-838). The job repairs the
source's plain row below the drained nodes' tight out-links. The reference for
every row is the oracle's runSpf on a topology loaded with isOverloaded set on
the request's drained nodes: metric and first-hop set of every node,
unreached nodes absent.
"""
import ctypes as C
import dataclasses
import random

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid, int_topology
from openr_amd.types import K_TESTING_AREA

from helpers import row_digest
from test_gpu_parity import random_topology

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
INF = 0xFFFFFFFF


class Oracles:
    """The oracle LinkState per distinct drain set: the adjacency databases
    copied with isOverloaded=True on those nodes, loaded afresh."""

    def __init__(self, oracle, dbs):
        self.oracle, self.dbs, self.cache = oracle, dbs, {}

    def __call__(self, drain):
        key = frozenset(drain)
        if key not in self.cache:
            dbs = [dataclasses.replace(db, isOverloaded=True) if db.thisNodeName in key else db
                   for db in self.dbs]
            als, _ = load_topology(self.oracle, dbs, [])
            self.cache[key] = als[A]
        return self.cache[key]


def _view(names, nbrs, dist, nh):
    """A fetched row in run_spf_ignoring's form: {node: (metric, sorted first hops)}."""
    out = {}
    for v in np.nonzero(dist != INF)[0]:
        m = int(nh[v])
        out[names[v]] = (int(dist[v]), sorted(nbrs[b] for b in range(32) if m >> b & 1))
    for v in np.nonzero(dist == INF)[0]:
        assert nh[v] == 0, names[v]
    return out


def _run(ls, srcs, idx, ignore, drain, chunk=None, **kw):
    b = ls.what_if_batch(srcs, idx, ignore, chunk or max(len(idx), 1), drain=drain, **kw)
    b.run()
    b.sync()
    return b


def _check_rows(ls, batch, oracles, srcs, idx, ignore, drain, desc, which=None):
    names = ls.node_names()
    nbrs = {s: ls.neighbors(s) for s in srcs}
    for i in (range(len(idx)) if which is None else which):
        s = srcs[idx[i]]
        d, m = batch.fetch(i)
        ref = oracles(drain[i])._impl.run_spf_ignoring(s, [desc[l][:3] for l in ignore[i]])
        assert _view(names, nbrs[s], d, m) == ref, (i, s, drain[i], [desc[l] for l in ignore[i]])


@pytest.mark.parametrize("seed", range(6))
def test_drain_random_graphs(hip, oracle, seed):
    """Every node drained from each of 4 sources (the source itself, nodes
    overloaded already and cut-off nodes included), sets of 2-3 nodes, and one
    drained node mixed with 1-2 ignored links."""
    uniform = seed % 2 == 1
    dbs = random_topology(5000 + seed, n=28, extra=40, max_metric=1 if uniform else 12,
                          parallel=0.25, overload=0.1, link_overload=0.08)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    rng = random.Random(seed)
    links = ls.link_ids()
    desc = dict(links)
    lids = [lid for lid, _ in links]
    names = sorted(db.thisNodeName for db in dbs)
    srcs = rng.sample(names, 4)
    idx, ignore, drain = [], [], []
    for x in names:
        for k in range(len(srcs)):
            idx.append(k)
            ignore.append([])
            drain.append([x])
    single = len(idx)
    for _ in range(single // 4):
        idx.append(rng.randrange(len(srcs)))
        ignore.append([])
        drain.append(rng.sample(names, rng.choice((2, 3))))
    for _ in range(single // 4):
        idx.append(rng.randrange(len(srcs)))
        ignore.append(rng.sample(lids, rng.choice((1, 2))))
        drain.append([rng.choice(names)])
    b = _run(ls, srcs, idx, ignore, drain)
    _check_rows(ls, b, Oracles(oracle, dbs), srcs, idx, ignore, drain, desc)
    info = b.info()
    overloaded = {db.thisNodeName for db in dbs if db.isOverloaded}
    for i in range(single):
        if drain[i][0] == srcs[idx[i]] or drain[i][0] in overloaded:
            assert info[i] == 0, (i, drain[i], srcs[idx[i]])  # tier 0, nothing re-derived
    assert np.any(info[:single] != 0)


def _hand_graph():
    """0 is the source. X1 = 1 is on the only shortest path to X2 = 2 (0-1-2);
    X2 has the subtree 3, 4, 5 behind it and a longer entry 0-6-7-2; 7-3 enters
    the subtree without X2; 8, 9 hang off X1 with a longer way round 0-10-11-9."""
    return int_topology({
        0: [(1, 1), (6, 3), (10, 2)],
        1: [(0, 1), (2, 1), (8, 1)],
        2: [(1, 1), (3, 1), (5, 1), (7, 3)],
        3: [(2, 1), (4, 1), (7, 4)],
        4: [(3, 1), (5, 2)],
        5: [(2, 1), (4, 2)],
        6: [(0, 3), (7, 3)],
        7: [(6, 3), (2, 3), (3, 4)],
        8: [(1, 1), (9, 1)],
        9: [(8, 1), (11, 5)],
        10: [(0, 2), (11, 1)],
        11: [(10, 1), (9, 5)],
    })


def test_drained_node_below_a_drained_node(hip, oracle):
    """{X1, X2}: X2 is below X1, so it is in the affected set, re-derived (it
    moves to the long entry) and not expanded; its subtree hangs on its own
    cuts. Also {X2} and {X1} alone, and the same from the far source 9."""
    dbs = _hand_graph()
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    srcs = ["0", "9"]
    sets = [["1", "2"], ["2"], ["1"], ["2", "1", "2"], []]
    idx = [k for k in range(len(srcs)) for _ in sets]
    drain = [s for _ in srcs for s in sets]
    ignore = [[] for _ in idx]
    b = _run(ls, srcs, idx, ignore, drain)
    _check_rows(ls, b, Oracles(oracle, dbs), srcs, idx, ignore, drain, {})
    names = ls.node_names()
    d, m = b.fetch(0)  # source 0, {X1, X2}
    row = _view(names, ls.neighbors("0"), d, m)
    assert row["1"] == (1, ["1"]) and row["2"] == (9, ["6"]) and row["3"] == (10, ["6"])
    info = b.info()
    assert info[0] & 7 == 1 and info[0] >> 3 >= 6  # 2, 8, 9, 3, 4, 5 at least
    assert info[4] == 0  # no drain: the base row


@pytest.mark.parametrize("use_link_metric", [True, False])
def test_drain_shrinks_the_ecmp_set(hip, oracle, use_link_metric):
    """6x6 unit grid, corner source 0, its neighbour 1 drained: interior
    nodes keep their distance and lose the first hop 1, the rest of row 0 gets
    longer, node 1 itself keeps {1}."""
    dbs, _ = bench_grid(6, 0)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    names = ls.node_names()
    nbrs = ls.neighbors("0")
    b = _run(ls, ["0"], [0, 0], [[], []], [["1"], []], use_link_metric=use_link_metric)
    got = _view(names, nbrs, *b.fetch(0))
    base = _view(names, nbrs, *b.fetch(1))
    oracles = Oracles(oracle, dbs)
    for row, drain in ((got, ["1"]), (base, [])):
        ref = oracles(drain).get_spf_result("0", use_link_metric)
        assert row == {k: (v.metric, sorted(v.nextHops)) for k, v in ref.items()}
    assert got["1"] == (1, ["1"])
    for r in range(6):
        for c in range(6):
            v = str(r * 6 + c)
            if r >= 1 and c >= 1:
                assert got[v] == (base[v][0], ["6"]) and base[v][1] == ["1", "6"]
            elif r == 0 and c >= 2:
                assert got[v] == (base[v][0] + 2, ["6"])
            elif v != "1":
                assert got[v] == base[v]
    assert b.info()[0] & 7 == 1 and b.info()[0] >> 3 == 29  # rows 1..5 x cols 1..5, and 2..5 of row 0


def test_disconnecting_drain(hip, oracle):
    """Node 3 is the single attachment of the stub {4, 5}: drained, it stays
    reached and the stub becomes unreached."""
    dbs = int_topology({
        0: [(1, 2), (2, 3)], 1: [(0, 2), (2, 1), (3, 4)], 2: [(0, 3), (1, 1)],
        3: [(1, 4), (4, 1), (5, 2)], 4: [(3, 1), (5, 1)], 5: [(3, 2), (4, 1)],
    })
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    srcs = ["0", "4"]
    idx, drain = [0, 1, 0], [["3"], ["3"], ["1"]]
    ignore = [[], [], []]
    b = _run(ls, srcs, idx, ignore, drain)
    _check_rows(ls, b, Oracles(oracle, dbs), srcs, idx, ignore, drain, {})
    names = ls.node_names()
    d, m = b.fetch(0)
    row = _view(names, ls.neighbors("0"), d, m)
    assert set(row) == {"0", "1", "2", "3"} and row["3"] == (6, ["1"])
    assert d[names.index("4")] == INF and d[names.index("5")] == INF
    # from inside the stub the drained attachment is the end of the world
    assert set(_view(names, ls.neighbors("4"), *b.fetch(1))) == {"3", "4", "5"}


def test_drain_tiers(hip, oracle):
    """60x60 grid (3,600 nodes), sources 0 (corner) and 1830 (centre).
    Draining 1 from 0 re-derives every node outside column 0 but 1 itself (3,539): more
    than the LDS tiers hold, so it is repaired in a global slot (tier 3), and
    70 copies of it pass the 64 slots (the slot tier is a queue, the extra
    ones wait for a free slot). Draining 1831 from 1830 re-derives columns
    31..59 but 1831 itself (1,739 nodes, under 6,800 predecessor edges): past tier 1's 256 nodes and
    within the 2,048 nodes / 8,192 edges that the repair state is sized to
    when it fits the LDS, as it does for a 3,600-node graph on this part
    (160 KB per workgroup), so this job shows tier 2; a job with slots reaches
    tier 4 only with search_large, checked last. 42 nodes near the far corner
    give small sets (tier 1), the corner itself none (tier 0)."""
    dbs, _ = bench_grid(60, 0)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    srcs = ["0", "1830"]
    far = [str(r * 60 + c) for r in range(54, 60) for c in range(53, 60)]
    reqs = [(0, "1")] * 35 + [(1, "1831")] + [(0, x) for x in far] + [(0, "1")] * 35
    idx = [k for k, _ in reqs]
    drain = [[x] for _, x in reqs]
    ignore = [[] for _ in reqs]
    b = _run(ls, srcs, idx, ignore, drain)
    info = b.info()
    tier, affected = info & 7, info >> 3
    big = [i for i, r in enumerate(reqs) if r == (0, "1")]
    assert len(big) == 70
    assert np.all(tier[big] == 3) and np.all(affected[big] == 3539)
    assert tier[35] == 2 and affected[35] == 1739
    assert tier[36 + far.index("3599")] == 0
    assert np.all(tier[36:36 + len(far) - 1] == 1)
    assert set(int(t) for t in tier) == {0, 1, 2, 3}
    first = {}
    for i, r in enumerate(reqs):
        first.setdefault(r, i)
    oracles = Oracles(oracle, dbs)
    _check_rows(ls, b, oracles, srcs, idx, ignore, drain, {}, which=sorted(first.values()))
    rows = {i: b.fetch(i) for i in range(len(reqs))}
    for i in big[1:]:
        assert np.array_equal(rows[i][0], rows[big[0]][0]) and np.array_equal(rows[i][1], rows[big[0]][1])
    del b
    s = _run(ls, srcs, idx, ignore, drain, search_large=True)
    assert np.any((s.info() & 7) == 4)
    for i in range(len(reqs)):
        d, m = s.fetch(i)
        assert np.array_equal(d, rows[i][0]) and np.array_equal(m, rows[i][1]), (i, reqs[i])


def _oracle_digests(oracles, ls, srcs, idx, drain):
    """row_digest of the oracle's row per request (spf_tables per drain set)."""
    names = ls.node_names()
    nbrs = [ls.neighbors(s) for s in srcs]
    tables, out = {}, []
    for i in range(len(idx)):
        key = frozenset(drain[i])
        if key not in tables:
            dist, nh = oracles(drain[i])._impl.spf_tables(srcs, names, nbrs, 4)
            tables[key] = (dist, nh[:, :, 0])
        dist, nh = tables[key]
        out.append(row_digest(dist[idx[i]], nh[idx[i]]))
    return np.array(out, dtype=np.uint64)


def test_drain_job_plumbing(hip, oracle):
    """Chunks smaller than the job (drain sets straddle chunk boundaries),
    digests, share_base, and a refresh after a metric change."""
    dbs = random_topology(5100, n=28, extra=40, max_metric=12, parallel=0.25, overload=0.1,
                          link_overload=0.08)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    names = sorted(db.thisNodeName for db in dbs)
    rng = random.Random(51)
    srcs = rng.sample(names, 4)
    idx = [k for _ in names for k in range(len(srcs))]
    drain = [[x] if n % 3 else [x, rng.choice(names)] for n, x in enumerate(names) for _ in srcs]
    ignore = [[] for _ in idx]
    oracles = Oracles(oracle, dbs)
    ref = _oracle_digests(oracles, ls, srcs, idx, drain)

    one = _run(ls, srcs, idx, ignore, drain)
    info = one.info()
    assert np.any((info & 7) == 0) and np.any((info & 7) != 0)
    b = ls.what_if_batch(srcs, idx, ignore, 10, drain=drain)  # 112 requests in chunks of 10
    b.set_digests()
    b.run()
    b.sync()
    assert np.array_equal(b.info(), info)
    assert np.array_equal(b.digests(), ref)

    sh = ls.what_if_batch(srcs, idx, ignore, len(idx), share_base=True, drain=drain)
    sh.set_digests()
    sh.run()
    sh.sync()
    assert np.array_equal(sh.info(), info)
    assert np.array_equal(sh.digests(), ref)
    for i in range(len(idx)):  # repaired rows from the buffer, standing ones from the base rows
        d, m = sh.fetch(i)
        assert row_digest(d, m) == int(ref[i]), (i, drain[i], int(info[i]))

    # a metric change, then run() refreshes the base rows on the new graph
    db = next(d for d in dbs if d.thisNodeName == srcs[0])
    adjs = [dataclasses.replace(a, metric=a.metric + 7) if k == 0 else a for k, a in enumerate(db.adjacencies)]
    new_db = dataclasses.replace(db, adjacencies=adjs)
    als_h[A].update_adjacency_database(new_db)
    dbs2 = [new_db if d.thisNodeName == srcs[0] else d for d in dbs]
    ref2 = _oracle_digests(Oracles(oracle, dbs2), ls, srcs, idx, drain)
    assert not np.array_equal(ref2, ref)
    b.run()
    b.sync()
    assert np.array_equal(b.digests(), ref2)


def test_drain_unknown_node_name(hip):
    dbs, _ = bench_grid(4, 0)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    with pytest.raises(ValueError, match="unknown drained node"):
        ls.what_if_batch(["0"], [0], [[]], 1, drain=[["no-such-node"]])
    with pytest.raises(ValueError, match="one drain set per request"):
        ls.what_if_batch(["0"], [0, 0], [[], []], 2, drain=[["1"]])


vp, u32p = C.c_void_p, C.POINTER(C.c_uint32)


class orh_csr(C.Structure):
    _fields_ = [("n_nodes", C.c_uint32), ("n_edges", C.c_uint32), ("n_links", C.c_uint32),
                ("row_ptr", vp), ("col", vp), ("w_out", vp), ("w_in", vp), ("meta", vp),
                ("node_overloaded", vp), ("name_rank", vp)]


def _p(a):
    return a.ctypes.data_as(vp)


def test_drain_c_abi(hip):
    """The raw library, as test_abi.py loads it, on a 5-node ring 0-1-2-3-4-0
    with unit metrics: a drained node id == N is ORH_E_INVALID with a message
    and queues nothing (the next, valid, run on the same job succeeds and is
    right); h_drain_ptr == NULL gives orh_whatif_run's rows byte for byte."""
    from openr_amd import HIP_LIB_PATH
    lib = C.CDLL(HIP_LIB_PATH)
    N = 5
    for name, args in {
        "orh_create": [C.c_int, C.c_uint32, C.POINTER(vp)], "orh_destroy": [vp],
        "orh_graph_create": [vp, C.POINTER(vp)], "orh_graph_destroy": [vp],
        "orh_graph_load": [vp, C.POINTER(orh_csr)],
        "orh_device_alloc": [vp, C.c_size_t, C.POINTER(vp)], "orh_device_free": [vp, vp],
        "orh_memcpy_d2h": [vp, vp, vp, C.c_size_t],
        "orh_whatif_create": [vp, vp, C.c_uint32, C.c_int32, C.POINTER(vp)],
        "orh_whatif_run": [vp, C.c_uint32, vp, vp, vp, vp, vp, vp],
        "orh_whatif_run_drains": [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, vp, vp],
        "orh_whatif_flush": [vp], "orh_whatif_destroy": [vp],
    }.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    lib.orh_last_error.argtypes, lib.orh_last_error.restype = [vp], C.c_char_p
    # link l joins l and (l + 1) % N; node v's entries: v - 1 (link v - 1), v + 1 (link v)
    row_ptr = np.arange(0, 2 * N + 1, 2, dtype=np.uint32)
    ents = [sorted([((v - 1) % N, (v - 1) % N), ((v + 1) % N, v)]) for v in range(N)]  # (col, link) by col
    col = np.array([c for row in ents for c, _ in row], np.uint32)
    meta = np.array([l for row in ents for _, l in row], np.uint32)
    w = np.ones(2 * N, np.uint32)
    ovl = np.zeros(N, np.uint8)
    csr = orh_csr(N, 2 * N, N, _p(row_ptr), _p(col), _p(w), _p(w), _p(meta), _p(ovl), None)
    ctx, g, job = vp(), vp(), vp()
    assert lib.orh_create(0, 0, C.byref(ctx)) == 0
    try:
        assert lib.orh_graph_create(ctx, C.byref(g)) == 0
        assert lib.orh_graph_load(g, C.byref(csr)) == 0, lib.orh_last_error(ctx)
        src = np.array([0], np.uint32)
        assert lib.orh_whatif_create(g, _p(src), 1, 1, C.byref(job)) == 0, lib.orh_last_error(ctx)
        n_req = 3
        bufs = []
        for _ in range(5):
            d = vp()
            assert lib.orh_device_alloc(ctx, n_req * N * 4, C.byref(d)) == 0
            bufs.append(d)
        d_dist, d_nh, d_info, d_dist2, d_nh2 = bufs

        def get(d, count):
            a = np.zeros(count, np.uint32)
            assert lib.orh_memcpy_d2h(ctx, _p(a), d, a.nbytes) == 0
            return a

        idx = np.zeros(n_req, np.uint32)
        ign_ptr = np.array([0, 0, 0, 1], np.uint32)  # request 2 ignores link 0 (0-1)
        ign = np.array([0], np.uint32)
        bad_ptr = np.array([0, 1, 2, 2], np.uint32)
        bad = np.array([1, N], np.uint32)
        rc = lib.orh_whatif_run_drains(job, n_req, _p(idx), _p(ign_ptr), _p(ign), _p(bad_ptr), _p(bad),
                                       d_dist, d_nh, d_info)
        assert rc == -1  # ORH_E_INVALID
        assert lib.orh_last_error(ctx)
        drn_ptr = np.array([0, 1, 3, 3], np.uint32)
        drn = np.array([1, 4, 4], np.uint32)  # {1}, {4, 4}, {}
        rc = lib.orh_whatif_run_drains(job, n_req, _p(idx), _p(ign_ptr), _p(ign), _p(drn_ptr), _p(drn),
                                       d_dist, d_nh, d_info)
        assert rc == 0, lib.orh_last_error(ctx)
        assert lib.orh_whatif_flush(job) == 0
        dist = get(d_dist, n_req * N).reshape(n_req, N)
        nh = get(d_nh, n_req * N).reshape(n_req, N)
        # neighbours of 0 in ascending id: 1 (bit 0), 4 (bit 1)
        assert dist.tolist() == [[0, 1, 3, 2, 1], [0, 1, 2, 3, 1], [0, 4, 3, 2, 1]]
        assert nh.tolist() == [[0, 1, 2, 2, 2], [0, 1, 1, 1, 2], [0, 2, 2, 2, 2]]
        assert [int(x) & 7 for x in get(d_info, n_req)] == [1, 1, 1]
        # NULL drain pointer: orh_whatif_run
        assert lib.orh_whatif_run_drains(job, n_req, _p(idx), _p(ign_ptr), _p(ign), None, None,
                                         d_dist, d_nh, None) == 0, lib.orh_last_error(ctx)
        assert lib.orh_whatif_run(job, n_req, _p(idx), _p(ign_ptr), _p(ign), d_dist2, d_nh2, None) == 0
        assert lib.orh_whatif_flush(job) == 0
        assert get(d_dist, n_req * N).tobytes() == get(d_dist2, n_req * N).tobytes()
        assert get(d_nh, n_req * N).tobytes() == get(d_nh2, n_req * N).tobytes()
        assert get(d_dist, n_req * N).reshape(n_req, N).tolist() == \
            [[0, 1, 2, 2, 1], [0, 1, 2, 2, 1], [0, 4, 3, 2, 1]]
    finally:
        if job:
            lib.orh_whatif_destroy(job)
        if g:
            lib.orh_graph_destroy(g)
        lib.orh_destroy(ctx)


def test_drain_multi_device(hip):
    """MultiDeviceWhatIf with drains over 2 contexts on one GPU: each block
    gets its own requests' drains, and the union of the blocks equals the
    single job by tier, affected count and row digest."""
    dbs, _ = bench_grid(12, 0)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    names = ls.node_names()
    rng = random.Random(8)
    srcs = rng.sample(names, 6)
    lids = [lid for lid, _ in ls.link_ids()]
    idx, ignore, drain = [], [], []
    for x in rng.sample(names, 40):
        for k in range(len(srcs)):
            idx.append(k)
            ignore.append([rng.choice(lids)] if len(idx) % 5 == 0 else [])
            drain.append([] if len(idx) % 7 == 0 else [x])
    one = ls.what_if_batch(srcs, idx, ignore, 64, drain=drain)
    one.set_digests()
    one.run()
    one.sync()
    info1, dig1 = one.info(), one.digests()
    assert np.any((info1 & 7) != 0)
    rls = hip.module.ReplicatedLinkState(A, [0, 0])
    for db in dbs:
        rls.update_adjacency_database(db.to_wire())
    assert rls.replica(0).node_names() == names
    md = rls.what_if_batch(srcs, idx, ignore, 64, drain=drain)
    assert md.blocks == 2 and md.block_requests(0) + md.block_requests(1) == len(idx)
    md.set_digests()
    md.run()
    md.sync()
    assert np.array_equal(md.info(), info1)
    assert np.array_equal(md.digests(), dig1)
    # the same requests without their drains give other rows: the drains arrived
    plain = rls.what_if_batch(srcs, idx, ignore, 64)
    plain.set_digests()
    plain.run()
    plain.sync()
    assert not np.array_equal(plain.digests(), dig1)
