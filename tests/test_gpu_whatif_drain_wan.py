"""Node-drain what-if requests on the 50k-node WAN (``-m gpu``): the C4 drain
shape (openr_amd.workloads.c4_drain_job) at 64 nodes x 4 sources."""
import dataclasses

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.types import K_TESTING_AREA

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA


def test_drain_wan_50k(hip, oracle):
    """Every row (dist and first-hop mask) of a 64 x 4 drain job equals the
    product's plain path on the mutated graph - per drained node an
    updateAdjacencyDatabase with the overload bit set, a sweep of the 4
    sources, and the update back (pinned to the oracle with overloaded nodes
    at this size by test_wan_50k_hbm_kernel) - and the request that changes the
    most nodes equals the oracle's runSpf on a topology with that node
    overloaded."""
    from openr_amd.workloads import c4_drain_job, c4_wan
    adj, _ = c4_wan()
    als_h, _ = load_topology(hip, adj, [])
    ls = als_h[A]._impl
    names = ls.node_names()
    srcs, idx, ignore, drain = c4_drain_job(names, 64, 4)
    assert len(srcs) == 4 and len(idx) == 256 and all(len(d) == 1 and not g for d, g in zip(drain, ignore))
    job = ls.what_if_batch(srcs, idx, ignore, len(idx), drain=drain)
    job.run()
    job.sync()
    info = job.info()
    rows = [job.fetch(i) for i in range(len(idx))]
    del job
    by_name = {db.thisNodeName: db for db in adj}
    base = ls.sweep(srcs, True)
    base.run()
    base.sync()
    base_rows = [tuple(a.reshape(-1) for a in base.fetch(k)) for k in range(len(srcs))]
    changed = []
    for n in range(0, len(idx), len(srcs)):
        x = drain[n][0]
        als_h[A].update_adjacency_database(dataclasses.replace(by_name[x], isOverloaded=True))
        sw = ls.sweep(srcs, True)
        sw.run()
        sw.sync()
        for k in range(len(srcs)):
            i = n + k
            assert idx[i] == k and drain[i] == [x]
            d, m = (a.reshape(-1) for a in sw.fetch(k))
            np.testing.assert_array_equal(rows[i][0], d, err_msg=f"dist {srcs[k]} drain {x}")
            np.testing.assert_array_equal(rows[i][1], m, err_msg=f"nh {srcs[k]} drain {x}")
            n_changed = int(np.sum((d != base_rows[k][0]) | (m != base_rows[k][1])))
            assert n_changed <= int(info[i] >> 3) or int(info[i] & 7) == 4, (i, n_changed, int(info[i]))
            changed.append((n_changed, i))
        del sw
        als_h[A].update_adjacency_database(by_name[x])
    n_changed, i = max(changed)
    assert n_changed > 0
    x, s = drain[i][0], srcs[idx[i]]
    dbs = [dataclasses.replace(db, isOverloaded=True) if db.thisNodeName == x else db for db in adj]
    als_o, _ = load_topology(oracle, dbs, [])
    ref = als_o[A]._impl.run_spf_ignoring(s, [])
    nbrs = ls.neighbors(s)
    dist, nh = rows[i]
    got = {}
    for v in np.nonzero(dist != 0xFFFFFFFF)[0]:
        m = int(nh[v])
        got[names[v]] = (int(dist[v]), sorted(nbrs[b] for b in range(32) if m >> b & 1))
    assert got == ref
