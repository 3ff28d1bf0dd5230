"""The C4 cost-in job (openr_amd.workloads.c4_costin_job: the link job's 4,096
links x 64 sources on c4_wan() with those links costed out x10, each request
lowering its link back to the plain metrics from both ends) through one
what-if job in chunks of C4_WHATIF_CHUNK, with the link-failure job on the
plain graph from the same process for context:

    python tools/whatif_costin.py [--links 4096] [--srcs 64] [--factor 10]

One JSON line: per job the device ms (last_ms, median of 5 runs after a
warm-up), the tier histogram and the mean / max affected count. The cost-in
requests change nothing in stage 1, so a tier-5 word's count is |M|, the
nodes the lower pass re-derived; "past_lds_nodes" counts the tier-5 requests
whose M alone outgrows the pass's LDS node cap (2,048 where that state fits,
as it does on this graph), which therefore finished in a global slot - a
lower bound of the requests that did, since an edge list past 8,192 sends a
smaller M there too."""
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
from openr_amd.workloads import C4_WHATIF_CHUNK, c4_costin_job, c4_wan, c4_what_if_job  # noqa: E402

LDS_NODE_CAP = 2048


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
           "tiers": {str(t): int(np.sum(tier == t)) for t in range(6)},
           "past_lds_nodes": int(np.sum((tier == 5) & (affected > LDS_NODE_CAP))),
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
    out = {"tool": "whatif_costin", "graph_nodes": len(names), "chunk": args.chunk, "factor": args.factor}

    srcs, idx, sets = c4_what_if_job([lid for lid, _ in links], names, args.links, args.srcs)
    job = ls.what_if_batch(srcs, idx, sets, args.chunk)
    out["link_job"] = measure(job)
    del job
    costed, srcs, idx, ignore, lower = c4_costin_job(links, adj, names, args.links, args.srcs, args.factor)
    del als, ls
    als, _ = load_topology(hip, costed, [])
    ls = als[A]._impl
    assert ls.link_ids() == links, "the costed-out graph numbers its links differently"
    job = ls.what_if_batch(srcs, idx, ignore, args.chunk, lower=lower)
    out["costin_job"] = measure(job)
    del job
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
