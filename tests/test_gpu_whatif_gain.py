"""Two-sided what-if records (orh_whatif_gain, WhatIfBatch.set_gain / gain /
node_gain) against tests/gain_model.py (``-m gpu``).

A record says what a request does to its source's routes in both directions:
nodes lost, farther and nearer (and by how much), rehomed, narrowed and
widened, with optional per-node weights and per-node counters. The model is
applied to the oracle's rows on the small random graphs (the cases that
test_whatif_gain_model.py proves non-vacuous on the CPU) and to the job's own
fetched rows everywhere. Every field is compared exactly.
"""
import ctypes as C

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import int_topology
from openr_amd.types import K_TESTING_AREA

from gain_model import FIELDS, REC, SHARED, gain_classes, node_counts, records_of, zero_record
from impact_model import NO_NODE
from route_abi import E_INVALID, OK, Device
from test_gpu_whatif_drain import orh_csr
from test_gpu_whatif_lower import Requests
from test_whatif_gain_model import CASES, LOWERS_ONLY, case_weights, oracle_case, suite_conditions
from whatif_raise_model import link_key

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
TILE = 2048  # nodes of a row per workgroup of whatif_gain_kernel
LOWERED = 5  # ORH_WHATIF_TIER_LOWERED
NODE_FIELDS = ("worst_node", "best_node")


def assert_records(got, want, what=""):
    assert tuple(got) == FIELDS
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype, f
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, (what, f, bad[:8].tolist(), got[f][bad[:8]].tolist(), want[f][bad[:8]].tolist())


def assert_zero_records(got, which, what=""):
    for f in FIELDS:
        assert np.all(got[f][which] == (NO_NODE if f in NODE_FIELDS else 0)), (what, f)


def run_gain(rq, ls, srcs, weights=None, node_counts=True, **kw):
    b = rq.batch(ls, srcs, **kw)
    b.set_gain(True, weights, node_counts=node_counts)
    b.run()
    b.sync()
    return b


def fetched_classes(b, names, srcs, rq, base_of):
    """gain_classes per request from the job's own rows (one chunk);
    base_of[k]: a request of source k that changes nothing."""
    base = {k: b.fetch(i) for k, i in base_of.items()}
    return [gain_classes(*base[rq.idx[i]], *b.fetch(i), names.index(srcs[rq.idx[i]])) for i in range(len(rq))]


def hip_case(hip, oracle, seed, n):
    """The random case (seed, n) of the model test on the device: its
    requests by link id, then one request per source that changes nothing
    (the base rows)."""
    case = oracle_case(oracle, seed, n)
    ls = load_topology(hip, case.dbs, [])[0][A]._impl
    lid = {link_key(d): l for l, d in ls.link_ids()}
    rq = Requests()
    for k, ignore, drain, raises, lowers in case.reqs:
        rq.add(k, [lid[x] for x in ignore], drain, [(lid[x], e, m) for x, e, m in raises],
               [(lid[x], e, m) for x, e, m in lowers])
    bare = {k: rq.add(k) for k in range(len(case.srcs))}
    return case, ls, rq, bare


@pytest.mark.parametrize("seed,n", CASES)
def test_gain_random_graphs(hip, oracle, seed, n):
    """28 nodes: whole quads, the 16-byte path; 30: the scalar path."""
    case, ls, rq, bare = hip_case(hip, oracle, seed, n)
    names, srcs = ls.node_names(), case.srcs
    assert len(names) == n and (n % 4 == 0) == (n == 28)
    weights = case_weights(names, seed)
    w = [weights[x] for x in names]
    b = run_gain(rq, ls, srcs, weights)
    got, got_nodes = b.gain(), b.node_gain()
    n_fam = len(case.reqs)
    from_oracle = case.classes(names, {s: ls.neighbors(s) for s in srcs})
    from_rows = fetched_classes(b, names, srcs, rq, bare)
    assert_records({f: v[:n_fam] for f, v in got.items()}, records_of(from_oracle, w), ("oracle", seed, n))
    assert_records(got, records_of(from_rows, w), ("fetched", seed, n))
    assert_zero_records(got, list(bare.values()))
    for classes in (from_oracle, from_rows):
        for a, want in zip(got_nodes, node_counts(classes)):
            assert np.array_equal(a, want)
    assert all(a.any() for a in got_nodes)
    seen, both = suite_conditions([from_oracle])
    assert len(seen) == 6 and both
    tier = b.info() & 7
    assert np.any(tier == 0) and np.any(tier == LOWERED)
    assert got["nearer_weight"].max() > 0xFFFFFFFF  # the sums did pass 32 bits
    # without weights and node counters: the same classes, zero weights
    b.set_gain(True)
    b.run()
    b.sync()
    plain = dict(got, **{f: np.zeros_like(got[f]) for f in ("lost_weight", "moved_weight", "nearer_weight")})
    assert_records(b.gain(), plain, "no weights")
    with pytest.raises(RuntimeError):
        b.node_gain()


def test_gain_hop_count_job(hip, oracle):
    """A hop-count job ignores metrics: a request that only lowers leaves its
    source's row alone, so its record is the zero record; the requests with
    an ignored link or a drained node still move nodes."""
    case, ls, rq, bare = hip_case(hip, oracle, *CASES[0])
    names, srcs = ls.node_names(), case.srcs
    b = run_gain(rq, ls, srcs, case_weights(names, 1), use_link_metric=False)
    got = b.gain()
    lowers_only = [i for i in range(len(case.reqs)) if case.family(i) in LOWERS_ONLY]
    rest = [i for i in range(len(case.reqs)) if case.family(i) not in LOWERS_ONLY]
    assert len(lowers_only) > len(rq) // 2
    assert_zero_records(got, lowers_only + list(bare.values()))
    assert not got["nearer"].any() and not got["widened"][lowers_only].any()
    assert got["farther"][rest].any() and got["lost"][rest].any()
    base = {k: b.fetch(i) for k, i in bare.items()}
    w = [case_weights(names, 1)[x] for x in names]
    want = records_of([gain_classes(*base[rq.idx[i]], *b.fetch(i), names.index(srcs[rq.idx[i]])) for i in rest], w)
    assert_records({f: v[rest] for f, v in got.items()}, want, "hop count")


def test_gain_chunks(hip, oracle):
    """The same requests in 7 chunks (more than the three row buffers, so a
    chunk's summary is queued before its buffer's next run; the last one
    partial), also with shared base rows, and in one chunk."""
    case, ls, rq, _ = hip_case(hip, oracle, *CASES[0])
    srcs = case.srcs
    weights = case_weights(ls.node_names(), 1)
    one = run_gain(rq, ls, srcs, weights)
    want, want_nodes = one.gain(), one.node_gain()
    assert want["nearer"].any() and want["farther"].any() and want["lost"].any()
    chunk = (len(rq) + 6) // 7 + 1
    assert (len(rq) + chunk - 1) // chunk == 7 and len(rq) % chunk
    for kw in ({}, {"share_base": True}):
        many = run_gain(rq, ls, srcs, weights, chunk=chunk, **kw)
        assert_records(many.gain(), want, kw)
        for a, b in zip(many.node_gain(), want_nodes):
            assert np.array_equal(a, b) and a.any()
        assert np.array_equal(many.info(), one.info())
        # a second run of the same job starts its node counters from zero again
        many.run()
        many.sync()
        assert_records(many.gain(), want, ("again", kw))
        for a, b in zip(many.node_gain(), want_nodes):
            assert np.array_equal(a, b)
        # release() keeps the last run's summaries on the host
        many.release()
        assert_records(many.gain(), want, ("released", kw))
        for a, b in zip(many.node_gain(), want_nodes):
            assert np.array_equal(a, b)
        # and the job runs again afterwards
        many.run()
        many.sync()
        assert_records(many.gain(), want, ("after release", kw))
        del many


def _lid(ls, a, b):
    return next(lid for lid, d in ls.link_ids() if {d[0], d[2]} == {a, b})


def _grid_map(rows, cols, metric):
    adj = {v: [] for v in range(rows * cols)}
    for r in range(rows):
        for c in range(cols):
            v = r * cols + c
            if c + 1 < cols:
                adj[v].append((v + 1, metric)), adj[v + 1].append((v, metric))
            if r + 1 < rows:
                adj[v].append((v + cols, metric)), adj[v + cols].append((v, metric))
    return adj


@pytest.mark.parametrize("leaf", [False, True])
def test_gain_rows_longer_than_a_tile(hip, leaf):
    """70x71 grid with every metric 4, and a source S that hangs on the corner
    0 by one link of metric 100: 4,971 nodes, three tiles of the scalar path
    (N % 4 == 3); with a leaf behind S 4,972, the 16-byte path. Lowering S -> 0
    to 1 brings every grid node nearer by 99: whole tiles of 2,048 nearer nodes
    go through the packed counts. Two lowers far from the source, the smaller
    one first on the way, put the best node behind the first changed one."""
    rows, cols = 70, 71
    n_grid = rows * cols
    adj = _grid_map(rows, cols, 4)
    s = n_grid
    adj[s] = [(0, 100)]
    adj[0].append((s, 100))
    if leaf:
        adj[s].append((s + 1, 1))
        adj[s + 1] = [(s, 1)]
    ls = load_topology(hip, int_topology(adj), [])[0][A]._impl
    names = ls.node_names()
    n = len(names)
    assert n == n_grid + 1 + leaf and (n % 4 == 0) == leaf and n > 2 * TILE
    hang = (_lid(ls, str(s), "0"), str(s), 1)

    def right(v, value):
        return (_lid(ls, str(v), str(v + 1)), str(v), value)

    early, late = right(1 * cols + 1, 3), right(40 * cols + 40, 1)
    rq = Requests()
    for lower in ([], [hang], [early, late], [hang, late], [late]):
        rq.add(0, lower=lower)
    weights = {x: (int(x) * 40503 + 1) & 0xFFFFFFFF for x in names}
    b = run_gain(rq, ls, [str(s)], weights)
    classes = fetched_classes(b, names, [str(s)], rq, {0: 0})
    want = records_of(classes, [weights[x] for x in names])
    got = b.gain()
    assert_records(got, want)
    for a, w in zip(b.node_gain(), node_counts(classes)):
        assert np.array_equal(a, w)
    assert_zero_records(got, [0])
    assert got["nearer"][1] == n_grid > 2 * TILE and got["max_gain"][1] == 99 and got["sum_gain"][1] == 99 * n_grid
    assert got["nearer_weight"][1] > 0xFFFFFFFF and got["farther"][1] == got["lost"][1] == 0
    per_tile = np.bincount(np.nonzero(classes[1].nearer)[0] // TILE, minlength=3)
    assert per_tile.max() == TILE  # a tile in which every node is nearer
    assert got["max_gain"][2] == 4 and got["max_gain"][3] == 102 and got["max_gain"][4] == 3

    def late_best(c, best):
        changed = np.nonzero(c.nearer | c.rehomed | c.widened | c.narrowed)[0]
        return best != NO_NODE and changed.min() // TILE < best // TILE
    assert any(late_best(c, int(x)) for c, x in zip(classes, want["best_node"]))


def test_gain_mixed_hand_graph(hip):
    """Source 0. 3 is reached over 2 at 2 (0-1-3 costs 3) with 4-5-6 behind
    it; 7 hangs on 0 by a link of metric 5 with 8 behind it.
      a  2-3 ignored, 0 -> 7 lowered to 1: 3..6 one farther, 7 and 8 four nearer
      b  3 drained, the same lower: 4..6 lost, 7 and 8 nearer
      c  1 -> 3 lowered to 1: the ways to 3 tie, so 3..6 keep their distance
         and gain the hop 1 (rehomed and widened, nobody nearer)."""
    adj = {0: [(1, 1), (2, 1), (7, 5)], 1: [(0, 1), (3, 2)], 2: [(0, 1), (3, 1)], 3: [(1, 2), (2, 1), (4, 1)],
           4: [(3, 1), (5, 1)], 5: [(4, 1), (6, 1)], 6: [(5, 1)], 7: [(0, 5), (8, 1)], 8: [(7, 1)]}
    ls = load_topology(hip, int_topology(adj), [])[0][A]._impl
    names = ls.node_names()
    node = names.index
    low = (_lid(ls, "0", "7"), "0", 1)
    rq = Requests()
    rq.add(0)
    rq.add(0, ignore=[_lid(ls, "2", "3")], lower=[low])
    rq.add(0, drain=["3"], lower=[low])
    rq.add(0, lower=[(_lid(ls, "1", "3"), "1", 1)])
    weights = {x: 1 << int(x) for x in names}
    b = run_gain(rq, ls, ["0"], weights)
    got = b.gain()
    rec = [{f: int(got[f][i]) for f in FIELDS} for i in range(len(rq))]
    assert rec[0] == zero_record()
    below3, below7 = 8 + 16 + 32 + 64, 128 + 256
    assert rec[1] == dict(lost=0, farther=4, nearer=2, rehomed=0, narrowed=0, widened=0, max_stretch=1,
                          worst_node=min(node(x) for x in "3456"), max_gain=4, best_node=min(node("7"), node("8")),
                          sum_stretch=4, sum_gain=8, lost_weight=0, moved_weight=below3 + below7,
                          nearer_weight=below7)
    assert rec[2] == dict(lost=3, farther=0, nearer=2, rehomed=0, narrowed=0, widened=0, max_stretch=0,
                          worst_node=NO_NODE, max_gain=4, best_node=min(node("7"), node("8")), sum_stretch=0,
                          sum_gain=8, lost_weight=below3 - 8, moved_weight=below3 - 8 + below7,
                          nearer_weight=below7)
    assert rec[3] == dict(lost=0, farther=0, nearer=0, rehomed=4, narrowed=0, widened=4, max_stretch=0,
                          worst_node=NO_NODE, max_gain=0, best_node=NO_NODE, sum_stretch=0, sum_gain=0,
                          lost_weight=0, moved_weight=below3, nearer_weight=0)
    assert_records(got, records_of(fetched_classes(b, names, ["0"], rq, {0: 0}), [weights[x] for x in names]))
    lost, moved, nearer = b.node_gain()
    by_name = lambda a: {names[v]: int(a[v]) for v in np.nonzero(a)[0]}
    assert by_name(lost) == {"4": 1, "5": 1, "6": 1}
    assert by_name(nearer) == {"7": 2, "8": 2}
    assert by_name(moved) == {"3": 2, "4": 3, "5": 3, "6": 3, "7": 2, "8": 2}


def test_gain_agrees_with_impact_without_lowers(hip, oracle):
    """The random case without its lowers (ignored links, drained nodes and
    raises remain): the job's rows summarised both ways give the same nine
    shared fields and node counters, and nothing is nearer."""
    case, ls, rq, bare = hip_case(hip, oracle, *CASES[0])
    names, srcs = ls.node_names(), case.srcs
    weights = case_weights(names, 5)
    g = run_gain(rq, ls, srcs, weights, lowers=False)
    i = rq.batch(ls, srcs, lowers=False)
    i.set_impact(True, weights, node_counts=True)
    i.run()
    i.sync()
    assert np.array_equal(g.info(), i.info()) and not np.any((g.info() & 7) == LOWERED)
    for k in range(len(rq)):
        (gd, gm), (d, m) = g.fetch(k), i.fetch(k)
        assert np.array_equal(gd, d) and np.array_equal(gm, m)
    got, imp = g.gain(), i.impact()
    assert tuple(imp) == SHARED
    for f in SHARED:
        assert got[f].dtype == imp[f].dtype and np.array_equal(got[f], imp[f]), f
    assert imp["farther"].any() and imp["lost"].any() and imp["rehomed"].any() and imp["moved_weight"].any()
    for f in ("nearer", "max_gain", "sum_gain", "nearer_weight"):
        assert not got[f].any(), f
    assert np.all(got["best_node"] == NO_NODE)
    lost, moved, nearer = g.node_gain()
    assert np.array_equal(lost, i.node_impact()[0]) and np.array_equal(moved, i.node_impact()[1])
    assert moved.any() and not nearer.any()


def test_gain_multi_device(hip, oracle):
    """MultiDeviceWhatIf over 2 and 4 contexts on one GPU: records in the
    caller's request order and node counters summed over the blocks equal
    the single job's."""
    case, ls, rq, _ = hip_case(hip, oracle, *CASES[0])
    names, srcs = ls.node_names(), case.srcs
    weights = case_weights(names, 3)
    one = run_gain(rq, ls, srcs, weights, chunk=512)
    want, want_nodes = one.gain(), one.node_gain()
    assert want["nearer"].any() and want["widened"].any() and all(a.any() for a in want_nodes)
    for world in (2, 4):
        rls = hip.module.ReplicatedLinkState(A, [0] * world)
        for db in case.dbs:
            rls.update_adjacency_database(db.to_wire())
        assert rls.replica(0).node_names() == names
        assert dict(rls.replica(world - 1).link_ids()) == dict(ls.link_ids())
        md = rls.what_if_batch(srcs, rq.idx, rq.ignore, 512, drain=rq.drain, metric=rq.metric, lower=rq.lower)
        assert md.blocks == world
        md.set_gain(True, weights, node_counts=True)
        md.run()
        md.sync()
        assert_records(md.gain(), want, world)
        for a, b in zip(md.node_gain(), want_nodes):
            assert np.array_equal(a, b)
        with pytest.raises(RuntimeError):
            md.impact()


def test_gain_mode_rules(hip):
    adj = {0: [(1, 4), (2, 4)], 1: [(0, 4), (2, 4)], 2: [(0, 4), (1, 4)]}
    ls = load_topology(hip, int_topology(adj), [])[0][A]._impl
    low = [[(_lid(ls, "0", "1"), "0", 2)]]
    b = ls.what_if_batch(["0"], [0], [[]], 1, lower=low)
    with pytest.raises(RuntimeError):
        b.gain()  # no run at all
    b.run()
    b.sync()
    with pytest.raises(RuntimeError):
        b.gain()  # a run without the mode
    b.set_gain(True)
    b.set_impact(True)
    with pytest.raises(ValueError, match="impact and gain"):
        b.run()
    with pytest.raises(RuntimeError):
        b.gain()
    b.set_impact(False)
    b.run()
    b.sync()
    got = b.gain()
    assert got["nearer"].tolist() == [1] and got["max_gain"].tolist() == [2]
    assert got["best_node"].tolist() == [ls.node_names().index("1")]
    with pytest.raises(RuntimeError):
        b.impact()
    with pytest.raises(RuntimeError):
        b.node_gain()  # node counts were not asked for
    with pytest.raises(ValueError, match="unknown weighted node"):
        b.set_gain(True, {"no-such-node": 1})
    b.set_gain(False)
    b.set_impact(True)
    with pytest.raises(ValueError, match="impact"):  # impact mode still refuses lowers
        b.run()
    # without lowers the two modes alternate on one batch
    p = ls.what_if_batch(["0"], [0], [[_lid(ls, "0", "1")]], 1)
    p.set_impact(True)
    p.run()
    p.sync()
    assert p.impact()["farther"].tolist() == [1]
    p.set_impact(False)
    p.set_gain(True)
    p.run()
    p.sync()
    assert p.gain()["farther"].tolist() == [1] and p.gain()["max_stretch"].tolist() == [4]
    with pytest.raises(RuntimeError):
        p.impact()


# ---- the C boundary ---------------------------------------------------------
vp = C.c_void_p


class orh_whatif_gain_opts(C.Structure):
    _fields_ = [("d_weight", vp), ("d_node_lost", vp), ("d_node_moved", vp), ("d_node_nearer", vp)]


def _p(a):
    return a.ctypes.data_as(vp)


def test_gain_c_abi_shared_base_rows(hip):
    """The raw library on a 12-node ring with a chord, every metric 3, two
    sources. Per source: nothing; a lower to the current value; an effective
    lower of the record into the source, which changes nothing (tier 0, yet
    the request owns its row); every link lowered to 1 from both ends. A
    SHARE_BASE job runs into row buffers filled with 0xA5: the rows of the
    first two kinds stay garbage, so equal records prove they are not read."""
    from openr_amd import HIP_LIB_PATH
    lib = C.CDLL(HIP_LIB_PATH)
    dev = Device(lib)
    for name, args in {
        "orh_graph_create": [vp, C.POINTER(vp)], "orh_graph_destroy": [vp],
        "orh_graph_load": [vp, C.POINTER(orh_csr)],
        "orh_whatif_create": [vp, vp, C.c_uint32, C.c_int32, C.POINTER(vp)],
        "orh_whatif_set_flags": [vp, C.c_uint32],
        "orh_whatif_run_lowers": [vp, C.c_uint32] + [vp] * 12,
        "orh_whatif_gain": [vp, C.c_uint32, vp, vp, vp, vp, C.POINTER(orh_whatif_gain_opts), vp],
        "orh_whatif_flush": [vp], "orh_whatif_destroy": [vp],
    }.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = args, C.c_int
    N = 12
    # link l < N joins l and (l + 1) % N; link N is the chord 2-8
    ents = [[((v - 1) % N, (v - 1) % N), ((v + 1) % N, v)] for v in range(N)]
    ents[2].append((8, N))
    ents[8].append((2, N))
    ents = [sorted(row) for row in ents]
    row_ptr = np.zeros(N + 1, np.uint32)
    row_ptr[1:] = np.cumsum([len(r) for r in ents])
    col = np.array([c for row in ents for c, _ in row], np.uint32)
    meta = np.array([l for row in ents for _, l in row], np.uint32)
    w = np.full(len(col), 3, np.uint32)
    ovl = np.zeros(N, np.uint8)
    csr = orh_csr(N, len(col), N + 1, _p(row_ptr), _p(col), _p(w), _p(w), _p(meta), _p(ovl), None)
    ctx, g, dense, shared = dev.ctx, vp(), vp(), vp()
    try:
        dev.ok(lib.orh_graph_create(ctx, C.byref(g)))
        dev.ok(lib.orh_graph_load(g, C.byref(csr)))
        srcs = np.array([0, 5], np.uint32)
        dev.ok(lib.orh_whatif_create(g, _p(srcs), 2, 1, C.byref(dense)))
        dev.ok(lib.orh_whatif_create(g, _p(srcs), 2, 1, C.byref(shared)))
        dev.ok(lib.orh_whatif_set_flags(shared, 1))  # ORH_WHATIF_SHARE_BASE
        # the record into source 0 is 1 -> 0 (link 0 from node 1), into source 5 it is 4 -> 5 (link 4 from node 4)
        into = {0: (0, 1, 1), 1: (4, 4, 1)}
        reqs = []
        for k in range(2):
            reqs += [(k, []), (k, [(3, NO_NODE, 3)]), (k, [into[k]])] + [(k, [(l, NO_NODE, 1)]) for l in range(N + 1)]
        # from 0, 8 is reached over the chord at 9; 0-11-10-9-8 at 2 + 1 + 3 + 3 ties with it: 8 gains a hop
        reqs.append((0, [(11, NO_NODE, 2), (10, NO_NODE, 1)]))
        n_req = len(reqs)
        nothing = [i for i, (_, low) in enumerate(reqs) if not low]
        same = [i for i, (_, low) in enumerate(reqs) if low and low[0][2] == 3]
        no_change = [i for i, (k, low) in enumerate(reqs) if low == [into[k]]]
        idx = np.array([k for k, _ in reqs], np.uint32)
        zeros = np.zeros(n_req + 1, np.uint32)
        low_ptr = np.zeros(n_req + 1, np.uint32)
        low_ptr[1:] = np.cumsum([len(low) for _, low in reqs])
        lows = np.array([x for _, low in reqs for t in low for x in t] + [0, 0, 0], np.uint32)
        weight = np.array([0, 1, 0x80000000, 0xFFFFFFFF, 5, 0, 7, 0xC0000000, 9, 10, 0xFFFFFFFF, 12], np.uint32)
        d_w = dev.upload(weight)

        def get(d, count, dtype=np.uint32):
            a = np.zeros(count, dtype)
            dev.ok(lib.orh_memcpy_d2h(ctx, _p(a), d, a.nbytes))
            return a

        def run(job, with_info=True, node_arrays=(None, None, None)):
            d_dist, d_nh = dev.alloc(n_req * N * 4, 0xA5), dev.alloc(n_req * N * 4, 0xA5)
            d_info, d_out = dev.alloc(n_req * 4, 0xA5), dev.alloc(n_req * REC.itemsize, 0xA5)
            dev.ok(lib.orh_whatif_run_lowers(job, n_req, _p(idx), _p(zeros), _p(zeros), None, None, None, None,
                                             _p(low_ptr), _p(lows), d_dist, d_nh, d_info))
            opts = orh_whatif_gain_opts(d_w, *node_arrays)
            rc = lib.orh_whatif_gain(job, n_req, _p(idx), d_dist, d_nh, d_info if with_info else None,
                                     C.byref(opts), d_out)
            return rc, d_dist, d_nh, d_info, d_out

        d_nodes = [dev.upload(np.zeros(N, np.uint32)) for _ in range(3)]
        rc, d_dist, d_nh, d_info, d_out = run(dense, node_arrays=d_nodes)
        dev.ok(rc)
        recs = get(d_out, n_req, REC)
        dist, nh = get(d_dist, n_req * N).reshape(n_req, N), get(d_nh, n_req * N).reshape(n_req, N)
        info = get(d_info, n_req)
        assert not info[nothing + same + no_change].any() and np.any((info & 7) == LOWERED)
        classes = [gain_classes(dist[nothing[k]], nh[nothing[k]], dist[i], nh[i], int(srcs[k]))
                   for i, (k, _) in enumerate(reqs)]
        want = records_of(classes, weight)
        for f in FIELDS:
            assert np.array_equal(recs[f], want[f]), f
        assert recs["nearer"].any() and recs["widened"].any() and recs["nearer_weight"].max() > 0xFFFFFFFF
        assert not recs["lost"].any() and not recs["farther"].any()
        zero = np.zeros(1, REC)
        zero["worst_node"] = zero["best_node"] = NO_NODE
        for i in nothing + same + no_change:
            assert recs[i].tobytes() == zero.tobytes(), i
        want_nodes = node_counts(classes)
        for d, a in zip(d_nodes, want_nodes):
            assert np.array_equal(get(d, N), a)
        # d_info = NULL on the dense job: every row scanned, the same records; the node arrays accumulate
        opts = orh_whatif_gain_opts(d_w, *d_nodes)
        d_out2 = dev.alloc(n_req * REC.itemsize, 0xA5)
        dev.ok(lib.orh_whatif_gain(dense, n_req, _p(idx), d_dist, d_nh, None, C.byref(opts), d_out2))
        assert get(d_out2, n_req, REC).tobytes() == recs.tobytes()
        assert np.array_equal(get(d_nodes[2], N), 2 * want_nodes[2]) and want_nodes[2].any()
        # opts = NULL: no weights
        dev.ok(lib.orh_whatif_gain(dense, n_req, _p(idx), d_dist, d_nh, d_info, None, d_out2))
        bare = get(d_out2, n_req, REC)
        assert not bare["moved_weight"].any() and not bare["nearer_weight"].any()
        assert np.array_equal(bare["nearer"], recs["nearer"]) and np.array_equal(bare["best_node"], recs["best_node"])

        # the SHARE_BASE job: rows of requests without an effective lower are never written
        rc, s_dist, s_nh, s_info, s_out = run(shared)
        dev.ok(rc)
        assert get(s_out, n_req, REC).tobytes() == recs.tobytes()
        assert np.array_equal(get(s_info, n_req), info)
        garbage = get(s_dist, n_req * N).reshape(n_req, N)
        assert np.all(garbage[nothing + same] == 0xA5A5A5A5)
        assert np.array_equal(garbage[no_change], dist[no_change])  # an effective lower owns its row
        assert lib.orh_whatif_gain(shared, n_req, _p(idx), s_dist, s_nh, None, None, s_out) == E_INVALID
        assert b"orh_whatif_gain" in lib.orh_last_error(ctx)

        # validation: nothing is queued, the output keeps its bytes
        d_out3 = dev.alloc(n_req * REC.itemsize, 0xA5)
        bad = idx.copy()
        bad[3] = 2
        assert lib.orh_whatif_gain(dense, n_req, _p(bad), d_dist, d_nh, d_info, None, d_out3) == E_INVALID
        assert b"orh_whatif_gain: source index" in lib.orh_last_error(ctx)
        assert lib.orh_whatif_gain(dense, n_req, _p(idx), d_dist, d_nh, d_info, None, None) == E_INVALID
        assert lib.orh_whatif_gain(dense, n_req, _p(idx), None, d_nh, d_info, None, d_out3) == E_INVALID
        assert lib.orh_whatif_gain(None, n_req, _p(idx), d_dist, d_nh, d_info, None, d_out3) == E_INVALID
        assert lib.orh_whatif_gain(dense, 0, None, None, None, None, None, None) == OK
        dev.ok(lib.orh_sync(ctx))
        assert np.all(get(d_out3, n_req * REC.itemsize, np.uint8) == 0xA5)
    finally:
        for job in (dense, shared):
            if job:
                lib.orh_whatif_destroy(job)
        if g:
            lib.orh_graph_destroy(g)
        dev.close()
