"""The C4 cost-out job (openr_amd.workloads.c4_costout_job: the link job's
4,096 links x 64 sources on c4_wan(), each link's metric raised x10 from both
ends instead of the link ignored) through one what-if job in chunks of
C4_WHATIF_CHUNK, with the link-failure job from the same process for context:

    python tools/whatif_costout.py [--links 4096] [--srcs 64] [--factor 10]

One JSON line: per job the device ms (last_ms, median of 5 runs after a
warm-up), the tier histogram and the mean / max affected count. A run with
raises takes no full search, so tier 4 stays empty."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from openr_amd import host_backend  # noqa: E402
from openr_amd.facade import load_topology  # noqa: E402
from openr_amd.types import K_TESTING_AREA as A  # noqa: E402
from openr_amd.workloads import C4_WHATIF_CHUNK, c4_costout_job, c4_wan, c4_what_if_job  # noqa: E402


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
    ap.add_argument("--links", type=int, default=4096)
    ap.add_argument("--srcs", type=int, default=64)
    ap.add_argument("--factor", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=C4_WHATIF_CHUNK)
    args = ap.parse_args()

    hip = host_backend()
    adj, _ = c4_wan()
    als, _ = load_topology(hip, adj, [])
    ls = als[A]._impl
    names = ls.node_names()
    links = ls.link_ids()
    out = {"tool": "whatif_costout", "graph_nodes": len(names), "chunk": args.chunk, "factor": args.factor}

    srcs, idx, sets = c4_what_if_job([lid for lid, _ in links], names, args.links, args.srcs)
    job = ls.what_if_batch(srcs, idx, sets, args.chunk)
    out["link_job"] = measure(job)
    del job
    srcs, idx, ignore, metric = c4_costout_job(links, adj, names, args.links, args.srcs, args.factor)
    job = ls.what_if_batch(srcs, idx, ignore, args.chunk, metric=metric)
    out["costout_job"] = measure(job)
    del job
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
