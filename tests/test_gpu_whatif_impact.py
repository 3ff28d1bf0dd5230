"""What-if impact records (orh_whatif_impact, WhatIfBatch.set_impact /
impact / node_impact) against tests/impact_model.py (``-m gpu``).

A record says what a request's link failure or node drain does to its source's
routes: nodes lost, farther (and by how much), rehomed, narrowed, with optional
per-node weights and per-node counters. The model is applied to the oracle's
rows on small graphs, and to the job's own fetched rows on the large grids
(whose rows other tests pin). Every field is compared exactly.
"""
import ctypes as C
import random

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid, int_topology
from openr_amd.types import K_TESTING_AREA

from impact_model import FIELDS, INF, NO_NODE, impact_classes, impact_record, node_counts
from route_abi import E_INVALID, E_STATE, OK, Device
from test_gpu_parity import random_topology
from test_gpu_whatif_drain import Oracles, orh_csr

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
TILE = 2048  # nodes of a row per workgroup of whatif_impact_kernel


def canon(d):
    """A link descriptor (n1, if1, n2, if2) whichever end comes first."""
    return tuple(sorted(((d[0], d[1]), (d[2], d[3]))))


def make_requests(names, n_links, seed):
    """4 sources; every link cut singly and every node drained singly from each
    source; two- and three-element sets of links, of nodes, and mixed. Links
    are indices into the canonically sorted descriptor list."""
    rng = random.Random(seed)
    srcs = rng.sample(names, 4)
    idx, ignore, drain = [], [], []
    for l in range(n_links):
        for k in range(4):
            idx.append(k), ignore.append([l]), drain.append([])
    for x in names:
        for k in range(4):
            idx.append(k), ignore.append([]), drain.append([x])
    for _ in range(16):
        idx.append(rng.randrange(4)), ignore.append(rng.sample(range(n_links), rng.choice((2, 3)))), drain.append([])
    for _ in range(16):
        idx.append(rng.randrange(4)), ignore.append([]), drain.append(rng.sample(names, rng.choice((2, 3))))
    for _ in range(16):
        idx.append(rng.randrange(4)), ignore.append(rng.sample(range(n_links), 2)), drain.append([rng.choice(names)])
    return srcs, idx, ignore, drain


def make_weights(names, seed):
    """Per-node weights with zeros and values >= 2^31: sums pass 32 bits."""
    rng = random.Random(seed + 77)
    return {x: rng.choice((0, 1, 64, 0x80000000, 0xFFFFFFFF, rng.randrange(1 << 32))) for x in names}


def to_row(ref, names, nbrs):
    """run_spf_ignoring's {node: (metric, first hops)} as (dist, mask) arrays."""
    pos = {x: i for i, x in enumerate(names)}
    bit = {x: b for b, x in enumerate(nbrs)}
    dist, nh = np.full(len(names), INF, np.uint32), np.zeros(len(names), np.uint32)
    for v, (metric, hops) in ref.items():
        dist[pos[v]] = metric
        nh[pos[v]] = sum(1 << bit[h] for h in hops)
    return dist, nh


def oracle_classes(oracles, descs, names, nbrs_of, srcs, idx, ignore, drain):
    """impact_classes per request from the oracle's rows; also the base rows'
    node id of each source."""
    base = {s: to_row(oracles([])._impl.run_spf_ignoring(s, []), names, nbrs_of[s]) for s in srcs}
    out = []
    for i in range(len(idx)):
        s = srcs[idx[i]]
        ref = oracles(drain[i])._impl.run_spf_ignoring(s, [tuple(descs[l][:3]) for l in ignore[i]])
        out.append(impact_classes(*base[s], *to_row(ref, names, nbrs_of[s]), names.index(s)))
    return out


def records_of(classes, weight):
    """Model records (dict of arrays keyed by FIELDS) from impact_classes results."""
    recs = {f: [] for f in FIELDS}
    w = np.asarray(weight, np.uint64)
    for lost, farther, rehomed, narrowed, stretch in classes:
        moved = lost | farther | rehomed
        far = bool(farther.any())
        for f, x in zip(FIELDS, (lost.sum(), farther.sum(), rehomed.sum(), narrowed.sum(),
                                 stretch.max() if far else 0, np.argmax(stretch) if far else NO_NODE,
                                 stretch.sum(), w[lost].sum(dtype=np.uint64), w[moved].sum(dtype=np.uint64))):
            recs[f].append(int(x))
    return {f: np.array(v, np.uint64 if "weight" in f or f == "sum_stretch" else np.uint32)
            for f, v in recs.items()}


def assert_records(got, want, what=""):
    assert tuple(got) == FIELDS
    for f in FIELDS:
        assert got[f].dtype == want[f].dtype, f
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, (what, f, bad[:8].tolist(), got[f][bad[:8]].tolist(), want[f][bad[:8]].tolist())


def conditions(classes):
    """(some lost, some rehomed without farther, some tie for max_stretch)."""
    lost = any(c[0].any() for c in classes)
    rehomed_only = any(c[2].any() and not c[1].any() for c in classes)
    tie = any(c[1].any() and (c[4] == c[4].max()).sum() >= 2 for c in classes)
    return lost, rehomed_only, tie


def run_job(ls, srcs, idx, ignore, drain, weights, chunk=None, **kw):
    b = ls.what_if_batch(srcs, idx, ignore, chunk or max(len(idx), 1), drain=drain if any(drain) else None, **kw)
    b.set_impact(True, weights, node_counts=True)
    b.run()
    b.sync()
    return b


def random_case(hip, seed, n):
    dbs = random_topology(seed, n=n, extra=40, max_metric=1 if seed % 2 else 12, parallel=0.25, overload=0.1,
                          link_overload=0.08)
    als_h, _ = load_topology(hip, dbs, [])
    ls = als_h[A]._impl
    links = sorted(ls.link_ids(), key=lambda t: canon(t[1]))
    lids, descs = [lid for lid, _ in links], [d for _, d in links]
    srcs, idx, ignore, drain = make_requests(sorted(db.thisNodeName for db in dbs), len(lids), seed)
    return dbs, ls, lids, descs, srcs, idx, [[lids[l] for l in s] for s in ignore], ignore, drain


# seeds whose requests meet every condition below (checked on the CPU with the
# oracle's rows): 28 nodes is the scalar path, 32 the 16-byte one
@pytest.mark.parametrize("seed,n", [(6100, 28), (6101, 28), (6101, 32)])
def test_impact_random_graphs(hip, oracle, seed, n):
    dbs, ls, lids, descs, srcs, idx, ignore, ignore_l, drain = random_case(hip, seed, n)
    names = ls.node_names()
    assert ls.what_if_batch(srcs, [0], [[]], 1).nodes == n
    weights = make_weights(names, seed)
    b = run_job(ls, srcs, idx, ignore, drain, weights)
    classes = oracle_classes(Oracles(oracle, dbs), descs, names, {s: ls.neighbors(s) for s in srcs}, srcs, idx,
                             ignore_l, drain)
    want = records_of(classes, [weights[x] for x in names])
    assert_records(b.impact(), want, (seed, n))
    lost, moved = b.node_impact()
    want_lost, want_moved = node_counts(classes)
    assert np.array_equal(lost, want_lost) and np.array_equal(moved, want_moved)
    assert conditions(classes) == (True, True, True)
    tier = b.info() & 7
    assert np.any(tier == 0) and np.any(tier != 0)
    assert want["moved_weight"].max() > 0xFFFFFFFF  # the sums did pass 32 bits
    # without weights and node counters: the same classes, zero weights
    b.set_impact(True)
    b.run()
    b.sync()
    plain = dict(want, lost_weight=np.zeros_like(want["lost_weight"]),
                 moved_weight=np.zeros_like(want["moved_weight"]))
    assert_records(b.impact(), plain, "no weights")
    with pytest.raises(RuntimeError):
        b.node_impact()


def test_impact_chunks(hip):
    """The same requests in 8 chunks (more than the three row buffers, so a
    chunk's summary is queued before its buffer's next run) and in one."""
    _, ls, _, _, srcs, idx, ignore, _, drain = random_case(hip, 6100, 28)
    weights = make_weights(ls.node_names(), 1)
    one = run_job(ls, srcs, idx, ignore, drain, weights)
    chunk = (len(idx) + 7) // 8
    many = run_job(ls, srcs, idx, ignore, drain, weights, chunk=chunk)
    assert (len(idx) + chunk - 1) // chunk >= 7
    assert_records(many.impact(), one.impact())
    for a, b in zip(many.node_impact(), one.node_impact()):
        assert np.array_equal(a, b) and a.any()
    assert np.array_equal(many.info(), one.info())
    # a second run of the same job starts its node counters from zero again
    many.run()
    many.sync()
    assert_records(many.impact(), one.impact())
    assert np.array_equal(many.node_impact()[1], one.node_impact()[1])
    # release() keeps the last run's summaries on the host
    want = one.impact(), one.node_impact()
    one.release()
    assert_records(one.impact(), want[0])
    assert np.array_equal(one.node_impact()[0], want[1][0])


def _lid(ls, a, b):
    return next(lid for lid, d in ls.link_ids() if {d[0], d[2]} == {a, b})


def _grid_map(rows, cols):
    adj = {v: [] for v in range(rows * cols)}
    for r in range(rows):
        for c in range(cols):
            v = r * cols + c
            if c + 1 < cols:
                adj[v].append(v + 1), adj[v + 1].append(v)
            if r + 1 < rows:
                adj[v].append(v + cols), adj[v + cols].append(v)
    return adj


def test_impact_hand_graphs(hip):
    """The two cases tests/test_whatif_impact_model.py works by hand, end to
    end, and a bridge whose cut loses the chain behind it."""
    # 8-ring, source 0, 0-1 cut
    ls = load_topology(hip, int_topology({v: [(v - 1) % 8, (v + 1) % 8] for v in range(8)}), [])[0][A]._impl
    names = ls.node_names()
    b = run_job(ls, ["0"], [0, 0], [[_lid(ls, "0", "1")], []], [[], []], {x: 1 << int(x) for x in names})
    rec = {f: v.tolist() for f, v in b.impact().items()}
    assert [rec[f][0] for f in FIELDS] == [0, 3, 1, 1, 6, names.index("1"), 12, 0, 2 + 4 + 8 + 16]
    assert [rec[f][1] for f in FIELDS] == [0, 0, 0, 0, 0, NO_NODE, 0, 0, 0]
    lost, moved = b.node_impact()
    assert not lost.any() and sorted(names[v] for v in np.nonzero(moved)[0]) == ["1", "2", "3", "4"]
    # 3x3 grid, source 0, 0-1 cut: 1 and 2 tie, the smaller node id wins
    ls = load_topology(hip, int_topology(_grid_map(3, 3)), [])[0][A]._impl
    names = ls.node_names()
    b = run_job(ls, ["0"], [0], [[_lid(ls, "0", "1")]], [[]], None)
    rec = {f: v.tolist() for f, v in b.impact().items()}
    assert [rec[f][0] for f in FIELDS] == [0, 2, 4, 4, 2, min(names.index("1"), names.index("2")), 4, 0, 0]
    # 4-ring 0-1-2-3 with the chain 3-4-5-6 behind the bridge 3-4
    ring = {0: [1, 3], 1: [0, 2], 2: [1, 3], 3: [2, 0, 4], 4: [3, 5], 5: [4, 6], 6: [5]}
    ls = load_topology(hip, int_topology(ring), [])[0][A]._impl
    names = ls.node_names()
    w = {"4": 0xFFFFFFFF, "5": 0x80000000, "6": 3, "0": 1000, "3": 5}
    b = run_job(ls, ["0", "6"], [0, 1], [[_lid(ls, "3", "4")]] * 2, [[], []], w)
    rec = {f: v.tolist() for f, v in b.impact().items()}
    assert [rec[f][0] for f in FIELDS] == [3, 0, 0, 0, 0, NO_NODE, 0, 0x180000002, 0x180000002]
    assert [rec[f][1] for f in FIELDS] == [4, 0, 0, 0, 0, NO_NODE, 0, 1005, 1005]  # from 6: the ring is lost
    lost, moved = b.node_impact()
    assert np.array_equal(lost, moved) and lost.tolist() == [1] * 7  # 4, 5, 6 from 0; 0, 1, 2, 3 from 6
    with pytest.raises(ValueError, match="unknown weighted node"):
        b.set_impact(True, {"no-such-node": 1})


def _fetched_classes(b, names, srcs, idx, base_of):
    """impact_classes per request from the job's own rows (one chunk);
    base_of[k]: a request of source k with nothing ignored."""
    base = {k: b.fetch(i) for k, i in base_of.items()}
    return [impact_classes(*base[idx[i]], *b.fetch(i), names.index(srcs[idx[i]])) for i in range(len(idx))]


def test_impact_every_tier(hip):
    """60x60 grid (3,600 nodes: two tiles of the 16-byte path). Cutting 0-1
    from the corner 0 re-derives 3,540 nodes (a global slot, tier 3; 70 copies
    pass the 64 slots), 1830-1831 from the centre 1,740 (tier 2), links at the
    far corner a handful (tier 1), nothing ignored is tier 0; with search_large
    the big ones are searched in full (tier 4) and summarise alike."""
    dbs, _ = bench_grid(60, 0)
    ls = load_topology(hip, dbs, [])[0][A]._impl
    names = ls.node_names()
    srcs = ["0", "1830"]
    corner, centre = _lid(ls, "0", "1"), _lid(ls, "1830", "1831")
    small = [_lid(ls, a, b) for a, b in (("3598", "3599"), ("3539", "3599"), ("3597", "3598"), ("3479", "3539"))]
    reqs = [(0, [corner])] * 35 + [(1, [centre]), (0, []), (1, [])] + [(0, [l]) for l in small] + \
        [(0, [corner])] * 35 + [(1, [small[0]]), (0, [corner, centre])]
    idx, ignore = [k for k, _ in reqs], [s for _, s in reqs]
    drain = [[] for _ in reqs]
    weights = {x: (int(x) * 2654435761) & 0xFFFFFFFF for x in names}
    b = run_job(ls, srcs, idx, ignore, drain, weights)
    tier = b.info() & 7
    assert np.all(tier[:35] == 3) and tier[35] == 2 and tier[36] == 0 and tier[37] == 0
    assert np.all(tier[38:42] == 1)
    assert set(tier.tolist()) == {0, 1, 2, 3}
    classes = _fetched_classes(b, names, srcs, idx, {0: 36, 1: 37})
    want = records_of(classes, [weights[x] for x in names])
    assert_records(b.impact(), want, "tiers 0-3")
    assert want["farther"][0] == 59 and want["rehomed"][0] == 59 * 59 and want["max_stretch"][0] == 2
    assert want["farther"][35] == 29 and want["rehomed"][35] == 29 * 59
    lost, moved = b.node_impact()
    want_lost, want_moved = node_counts(classes)
    assert np.array_equal(lost, want_lost) and np.array_equal(moved, want_moved)
    # changed nodes in both tiles
    ids = np.nonzero(classes[0][1] | classes[0][2])[0]
    assert ids.min() < TILE <= ids.max()
    s = run_job(ls, srcs, idx, ignore, drain, weights, search_large=True)
    assert np.any((s.info() & 7) == 4)
    assert_records(s.impact(), want, "search_large")


def test_impact_rows_longer_than_a_tile(hip):
    """70x71 grid: 4,970 nodes, three tiles of the scalar path (N % 4 == 2).
    Cuts at both ends of the id range; one request's changed nodes lie in
    more than one tile with its worst node in a later one than its first
    changed node."""
    rows, cols = 70, 71
    n = rows * cols
    ls = load_topology(hip, int_topology(_grid_map(rows, cols)), [])[0][A]._impl
    names = ls.node_names()
    assert len(names) == n and n % 4 and n > 2 * TILE
    last = str(n - 1)
    srcs = ["0", last]
    cuts = [("0", "1"), ("0", str(cols)), (last, str(n - 2)), (last, str(n - 1 - cols)), ("2500", "2501")]
    reqs = [(0, []), (1, [])] + [(k, [_lid(ls, a, b)]) for k in range(2) for a, b in cuts]
    idx, ignore = [k for k, _ in reqs], [s for _, s in reqs]
    drain = [[] for _ in reqs]
    weights = {x: (int(x) * 40503 + 1) & 0xFFFFFFFF for x in names}
    b = run_job(ls, srcs, idx, ignore, drain, weights)
    classes = _fetched_classes(b, names, srcs, idx, {0: 0, 1: 1})
    want = records_of(classes, [weights[x] for x in names])
    assert_records(b.impact(), want)
    lost, moved = b.node_impact()
    want_lost, want_moved = node_counts(classes)
    assert np.array_equal(lost, want_lost) and np.array_equal(moved, want_moved)
    assert want["farther"].max() >= cols - 1 and want["rehomed"].max() > 2 * TILE

    def late_worst(c, worst):
        changed = np.nonzero(c[0] | c[1] | c[2] | c[3])[0]
        return worst != NO_NODE and changed.min() // TILE < worst // TILE
    assert any(late_worst(c, int(wn)) for c, wn in zip(classes, want["worst_node"]))


def test_impact_multi_device(hip):
    """MultiDeviceWhatIf over 2 and 4 contexts on one GPU: records in the
    caller's request order and node counters summed over the blocks equal
    the single job's."""
    dbs, _ = bench_grid(12, 0)
    ls = load_topology(hip, dbs, [])[0][A]._impl
    names = ls.node_names()
    rng = random.Random(9)
    srcs = rng.sample(names, 6)
    lids = [lid for lid, _ in ls.link_ids()]
    idx, ignore, drain = [], [], []
    for x in rng.sample(names, 30):
        for k in rng.sample(range(len(srcs)), len(srcs)):
            idx.append(k)
            ignore.append([rng.choice(lids)] if len(idx) % 3 else [])
            drain.append([] if len(idx) % 4 == 0 else [x])
    weights = make_weights(names, 3)
    one = run_job(ls, srcs, idx, ignore, drain, weights, chunk=64)
    want, want_nodes = one.impact(), one.node_impact()
    assert want["farther"].any() and want["rehomed"].any() and want_nodes[1].any()
    for world in (2, 4):
        rls = hip.module.ReplicatedLinkState(A, [0] * world)
        for db in dbs:
            rls.update_adjacency_database(db.to_wire())
        assert rls.replica(0).node_names() == names
        md = rls.what_if_batch(srcs, idx, ignore, 64, drain=drain)
        assert md.blocks == world
        md.set_impact(True, weights, node_counts=True)
        md.run()
        md.sync()
        assert_records(md.impact(), want, world)
        for a, b in zip(md.node_impact(), want_nodes):
            assert np.array_equal(a, b)
        assert np.array_equal(md.info() & 7 == 0, one.info() & 7 == 0)


# ---- the C boundary ---------------------------------------------------------
vp = C.c_void_p
REC = np.dtype([("lost", "<u4"), ("farther", "<u4"), ("rehomed", "<u4"), ("narrowed", "<u4"),
                ("max_stretch", "<u4"), ("worst_node", "<u4"), ("sum_stretch", "<u8"), ("lost_weight", "<u8"),
                ("moved_weight", "<u8")])
assert REC.itemsize == 48 and REC.names == FIELDS


class orh_whatif_impact_opts(C.Structure):
    _fields_ = [("d_weight", vp), ("d_node_lost", vp), ("d_node_moved", vp)]


def _p(a):
    return a.ctypes.data_as(vp)


def test_impact_c_abi_shared_base_rows(hip):
    """The raw library on a 12-node ring with a chord (unit metrics), two
    sources. A SHARE_BASE job runs into row buffers filled with 0xA5: its
    tier-0 rows stay garbage, so equal records prove they are not read."""
    from openr_amd import HIP_LIB_PATH
    lib = C.CDLL(HIP_LIB_PATH)
    dev = Device(lib)
    for name, args in {
        "orh_graph_create": [vp, C.POINTER(vp)], "orh_graph_destroy": [vp],
        "orh_graph_load": [vp, C.POINTER(orh_csr)],
        "orh_graph_apply_delta": [vp, C.c_uint32, vp, vp, vp, vp, vp, vp, C.c_uint32],
        "orh_whatif_create": [vp, vp, C.c_uint32, C.c_int32, C.POINTER(vp)],
        "orh_whatif_set_flags": [vp, C.c_uint32],
        "orh_whatif_run": [vp, C.c_uint32, vp, vp, vp, vp, vp, vp],
        "orh_whatif_impact": [vp, C.c_uint32, vp, vp, vp, vp, C.POINTER(orh_whatif_impact_opts), vp],
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
    w = np.ones(len(col), np.uint32)
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
        # every link from both sources, and three requests with nothing ignored
        reqs = [(k, [l]) for k in range(2) for l in range(N + 1)] + [(0, []), (1, []), (0, [])]
        n_req = len(reqs)
        idx = np.array([k for k, _ in reqs], np.uint32)
        ign_ptr = np.zeros(n_req + 1, np.uint32)
        ign_ptr[1:] = np.cumsum([len(s) for _, s in reqs])
        ign = np.array([l for _, s in reqs for l in s], np.uint32)
        weight = np.array([0, 1, 0x80000000, 0xFFFFFFFF, 5, 0, 7, 0xC0000000, 9, 10, 11, 12], np.uint32)
        d_w = dev.upload(weight)

        def run(job, with_info=True, node_arrays=None):
            d_dist, d_nh = dev.alloc(n_req * N * 4, 0xA5), dev.alloc(n_req * N * 4, 0xA5)
            d_info, d_out = dev.alloc(n_req * 4, 0xA5), dev.alloc(n_req * 48, 0xA5)
            dev.ok(lib.orh_whatif_run(job, n_req, _p(idx), _p(ign_ptr), _p(ign), d_dist, d_nh, d_info))
            opts = orh_whatif_impact_opts(d_w, *(node_arrays or (None, None)))
            rc = lib.orh_whatif_impact(job, n_req, _p(idx), d_dist, d_nh, d_info if with_info else None,
                                       C.byref(opts), d_out)
            return rc, d_dist, d_nh, d_info, d_out

        def get(d, count, dtype=np.uint32):
            a = np.zeros(count, dtype)
            dev.ok(lib.orh_memcpy_d2h(ctx, _p(a), d, a.nbytes))
            return a

        d_lost, d_moved = dev.upload(np.zeros(N, np.uint32)), dev.upload(np.zeros(N, np.uint32))
        rc, d_dist, d_nh, d_info, d_out = run(dense, node_arrays=(d_lost, d_moved))
        dev.ok(rc)
        recs = get(d_out, n_req, REC)
        dist, nh = get(d_dist, n_req * N).reshape(n_req, N), get(d_nh, n_req * N).reshape(n_req, N)
        tier = get(d_info, n_req) & 7
        assert tier[-3:].tolist() == [0, 0, 0] and np.any(tier != 0)
        base = {0: n_req - 3, 1: n_req - 2}
        classes = [impact_classes(dist[base[k]], nh[base[k]], dist[i], nh[i], int(srcs[k]))
                   for i, (k, _) in enumerate(reqs)]
        want = records_of(classes, weight)
        for f in FIELDS:
            assert np.array_equal(recs[f], want[f]), f
        assert recs["farther"].any() and recs["rehomed"].any() and recs["lost_weight"].max() == 0
        want_lost, want_moved = node_counts(classes)
        assert np.array_equal(get(d_lost, N), want_lost) and np.array_equal(get(d_moved, N), want_moved)
        # d_info = NULL on the dense job: every row scanned, the same records; the node arrays accumulate
        opts = orh_whatif_impact_opts(d_w, d_lost, d_moved)
        d_out2 = dev.alloc(n_req * 48, 0xA5)
        dev.ok(lib.orh_whatif_impact(dense, n_req, _p(idx), d_dist, d_nh, None, C.byref(opts), d_out2))
        assert get(d_out2, n_req, REC).tobytes() == recs.tobytes()
        assert np.array_equal(get(d_moved, N), 2 * want_moved)
        # opts = NULL: no weights
        dev.ok(lib.orh_whatif_impact(dense, n_req, _p(idx), d_dist, d_nh, d_info, None, d_out2))
        bare = get(d_out2, n_req, REC)
        assert not bare["moved_weight"].any() and np.array_equal(bare["farther"], recs["farther"])

        # the SHARE_BASE job: tier-0 rows are never written
        rc, s_dist, s_nh, s_info, s_out = run(shared)
        dev.ok(rc)
        assert get(s_out, n_req, REC).tobytes() == recs.tobytes()
        garbage = get(s_dist, n_req * N).reshape(n_req, N)
        assert np.all(garbage[-3:] == 0xA5A5A5A5)
        assert lib.orh_whatif_impact(shared, n_req, _p(idx), s_dist, s_nh, None, None, s_out) == E_INVALID
        assert b"orh_whatif_impact" in lib.orh_last_error(ctx)

        # validation: nothing is queued, the output keeps its bytes
        d_out3 = dev.alloc(n_req * 48, 0xA5)
        bad = idx.copy()
        bad[3] = 2
        assert lib.orh_whatif_impact(dense, n_req, _p(bad), d_dist, d_nh, d_info, None, d_out3) == E_INVALID
        assert b"orh_whatif_impact" in lib.orh_last_error(ctx)
        assert lib.orh_whatif_impact(dense, n_req, _p(idx), d_dist, d_nh, d_info, None, None) == E_INVALID
        assert lib.orh_whatif_impact(dense, n_req, _p(idx), None, d_nh, d_info, None, d_out3) == E_INVALID
        assert lib.orh_whatif_impact(None, n_req, _p(idx), d_dist, d_nh, d_info, None, d_out3) == E_INVALID
        assert lib.orh_whatif_impact(dense, 0, None, None, None, None, None, None) == OK
        # a structural delta (row 0 written again): the job no longer matches the graph
        r0 = slice(int(row_ptr[0]), int(row_ptr[1]))
        rows, ptr = np.array([0], np.uint32), np.array([0, r0.stop - r0.start], np.uint32)
        dev.ok(lib.orh_graph_apply_delta(g, 1, _p(rows), _p(ptr), _p(col[r0].copy()), _p(w[r0].copy()),
                                         _p(w[r0].copy()), _p(meta[r0].copy()), N + 1))
        assert lib.orh_whatif_impact(dense, n_req, _p(idx), d_dist, d_nh, d_info, None, d_out3) == E_STATE
        assert lib.orh_whatif_impact(dense, 0, None, None, None, None, None, None) == OK
        dev.ok(lib.orh_sync(ctx))
        assert np.all(get(d_out3, n_req * 48, np.uint8) == 0xA5)
    finally:
        for job in (dense, shared):
            if job:
                lib.orh_whatif_destroy(job)
        if g:
            lib.orh_graph_destroy(g)
        dev.close()
