"""The C4 cost-in job (openr_amd.workloads.c4_costin_job: the link job's 4,096
links x 64 sources on c4_wan() with those links costed out x10, each request
lowering its link back to the plain metrics from both ends) through one
what-if job in chunks of C4_WHATIF_CHUNK, with the link-failure job on the
plain graph from the same process for context:

    python tools/whatif_costin.py [--links 4096] [--srcs 64] [--factor 10] [--gain [--out FILE]]

One JSON line: per job the device ms (last_ms, median of 5 runs after a
warm-up), the tier histogram and the mean / max affected count. The cost-in
requests change nothing in stage 1, so a tier-5 word's count is |M|, the
nodes the lower pass re-derived; "past_lds_nodes" counts the tier-5 requests
whose M alone outgrows the pass's LDS node cap (2,048 where that state fits,
as it does on this graph), which therefore finished in a global slot - a
lower bound of the requests that did, since an edge list past 8,192 sends a
smaller M there too.

--gain measures every job again with the two-sided summaries (set_gain,
weighted by c4_node_weights, with node counts), the plain and the summarised
form alternated in one process after a warm-up of each: "gain_device_ms" and
the totals of nearer, widened, sum_gain and max_gain per job, and the cost of
the mode as added ms and as ms per GB of request rows scanned (requests with a
non-zero tier x N x 8 bytes; the cost-in job scans nearly every row, the link
job only the repaired ones, so the per-GB figures are the comparable ones).
The link job is summarised by set_impact the same way as the yardstick: its
rows have no nearer node, so both kernels read the same bytes there. --out
writes the JSON to a file as well."""
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
from openr_amd.workloads import (C4_WHATIF_CHUNK, c4_costin_job, c4_node_weights, c4_wan,  # noqa: E402
                                 c4_what_if_job)

LDS_NODE_CAP = 2048


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3), "runs_ms": [round(x, 3) for x in ms]}


def measure_modes(job, weights, n_nodes, modes, runs=5):
    """The job plain and in each summary mode of `modes` ("impact", "gain"),
    alternated run by run after a warm-up of each form. Per mode: the device
    ms, the ms it adds to the plain job, and that per GB of rows scanned."""
    def once(mode):
        job.set_impact(mode == "impact", weights if mode == "impact" else None, node_counts=mode == "impact")
        job.set_gain(mode == "gain", weights if mode == "gain" else None, node_counts=mode == "gain")
        job.run()
        job.sync()
        return job.last_ms()
    forms = ["off"] + list(modes)
    for f in forms:
        once(f)
    ms = {f: [] for f in forms}
    for _ in range(runs):
        for f in forms:
            ms[f].append(once(f))
    out = {}
    if forms[-1] == "gain":  # the last run's records
        rec = job.gain()
        _, _, nearer = job.node_gain()
        out.update({"nearer": int(rec["nearer"].sum()), "widened": int(rec["widened"].sum()),
                    "sum_gain": int(rec["sum_gain"].sum()), "max_gain": int(rec["max_gain"].max()),
                    "farther": int(rec["farther"].sum()), "lost": int(rec["lost"].sum()),
                    "requests_with_nearer": int(np.sum(rec["nearer"] > 0)),
                    "nodes_ever_nearer": int(np.sum(nearer > 0)),
                    "nearer_weight": int(rec["nearer_weight"].sum(dtype=np.uint64))})
    scanned = int(np.sum((job.info() & 7) != 0))
    gb = scanned * n_nodes * 8 / 1e9
    off = statistics.median(ms["off"])
    out.update({"scanned_requests": scanned, "scanned_gb": round(gb, 3), "off": spread(ms["off"])})
    for m in modes:
        added = statistics.median(ms[m]) - off
        out[m + "_device_ms"] = round(statistics.median(ms[m]), 3)
        out[m] = dict(spread(ms[m]), added_ms=round(added, 3), added_ms_per_gb=round(added / gb, 4) if gb else None,
                      floor_ms_per_gb_at_8TBps=0.125)
    return out


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
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=4096)
    ap.add_argument("--srcs", type=int, default=64)
    ap.add_argument("--factor", type=int, default=10)
    ap.add_argument("--chunk", type=int, default=C4_WHATIF_CHUNK)
    ap.add_argument("--gain", action="store_true", help="measure the jobs again with gain summaries")
    ap.add_argument("--out", help="write the JSON here as well")
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
    if args.gain:
        weights = c4_node_weights(names)
        out["link_job"].update(measure_modes(job, weights, len(names), ["impact", "gain"]))
    job.release()
    del job
    costed, srcs, idx, ignore, lower = c4_costin_job(links, adj, names, args.links, args.srcs, args.factor)
    del als, ls
    als, _ = load_topology(hip, costed, [])
    ls = als[A]._impl
    assert ls.link_ids() == links, "the costed-out graph numbers its links differently"
    job = ls.what_if_batch(srcs, idx, ignore, args.chunk, lower=lower)
    out["costin_job"] = measure(job)
    if args.gain:
        out["costin_job"].update(measure_modes(job, weights, len(names), ["gain"]))
    job.release()
    del job
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
