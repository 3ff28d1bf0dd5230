"""The C4 drain job (openr_amd.workloads.c4_drain_job: 4,096 drained nodes x
64 sources on c4_wan()) through one what-if job in chunks of C4_WHATIF_CHUNK,
with the link job of equal size from the same process for context:

    python tools/whatif_drain.py [--nodes 4096] [--srcs 64] [--baseline K]

One JSON line: per job the device ms (last_ms, median of 5 runs after a
warm-up), the tier histogram and the mean / max affected count. --baseline K
also times the only way to get these rows without drain requests, for K of
the seeded nodes: updateAdjacencyDatabase with the overload bit set, a sweep
of the sources, the update back; it reports the per-node time and its
extrapolation to the job's node count (an extrapolation, not a run)."""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from openr_amd import host_backend  # noqa: E402
from openr_amd.facade import load_topology  # noqa: E402
from openr_amd.types import K_TESTING_AREA as A  # noqa: E402
from openr_amd.workloads import C4_WHATIF_CHUNK, c4_drain_job, c4_wan, c4_what_if_job  # noqa: E402


def measure(job, runs=5):
    job.run()
    job.sync()
    ms = []
    for _ in range(runs):
        job.run()
        job.sync()
        ms.append(job.last_ms())
    info = job.info()
    tier, affected = info & 7, info >> 3
    repaired = affected[affected > 0]
    out = {"requests": int(len(info)), "device_ms": round(statistics.median(ms), 3),
           "device_ms_runs": [round(x, 3) for x in ms],
           "tiers": {str(t): int(np.sum(tier == t)) for t in range(5)},
           "affected_mean": round(float(affected.mean()), 2),
           "affected_mean_repaired": round(float(repaired.mean()), 2) if len(repaired) else 0.0,
           "affected_max": int(affected.max())}
    job.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=4096)
    ap.add_argument("--srcs", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=C4_WHATIF_CHUNK)
    ap.add_argument("--baseline", type=int, default=0, metavar="K")
    ap.add_argument("--link-only", action="store_true", help="the link job alone (A/B of the link path)")
    args = ap.parse_args()

    hip = host_backend()
    adj, _ = c4_wan()
    als, _ = load_topology(hip, adj, [])
    ls = als[A]._impl
    names = ls.node_names()
    out = {"tool": "whatif_drain", "graph_nodes": len(names), "chunk": args.chunk}

    srcs, idx, sets = c4_what_if_job([lid for lid, _ in ls.link_ids()], names, args.nodes, args.srcs)
    job = ls.what_if_batch(srcs, idx, sets, args.chunk)
    out["link_job"] = measure(job)
    del job
    if not args.link_only:
        srcs, idx, ignore, drain = c4_drain_job(names, args.nodes, args.srcs)
        job = ls.what_if_batch(srcs, idx, ignore, args.chunk, drain=drain)
        out["drain_job"] = measure(job)
        del job
        if args.baseline > 0:
            by_name = {db.thisNodeName: db for db in adj}
            nodes = [d[0] for d in drain[::len(srcs)]][:args.baseline]
            sw = ls.sweep(srcs, True)  # warm-up
            sw.run()
            sw.sync()
            del sw
            per = []
            for x in nodes:
                t0 = time.perf_counter()
                als[A].update_adjacency_database(dataclasses.replace(by_name[x], isOverloaded=True))
                sw = ls.sweep(srcs, True)  # a sweep object binds the mirror as patched
                sw.run()
                sw.sync()
                del sw
                als[A].update_adjacency_database(by_name[x])
                per.append((time.perf_counter() - t0) * 1e3)
            med = statistics.median(per)
            out["baseline"] = {"what": "per node: overload on, sweep of the sources, overload off (wall ms)",
                               "nodes_timed": len(nodes), "per_node_ms": round(med, 3),
                               "per_node_ms_range": [round(min(per), 3), round(max(per), 3)],
                               "extrapolated_ms_for_job": round(med * args.nodes, 1),
                               "extrapolated": True}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
