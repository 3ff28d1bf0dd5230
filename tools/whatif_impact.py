"""Impact summaries of the C4 what-if jobs (openr_amd.workloads: 4,096 links /
4,096 drained nodes x 64 sources on c4_wan(), c4_node_weights) on a GPU box:

    python tools/whatif_impact.py [--nodes 4096] [--srcs 64] [--reps 5] [--out FILE]

Per job: the ten requests with the largest lost_weight and moved_weight, and
the device time (last_ms) with impact off and on, the two alternated in one
process after a warm-up of each, median and range of --reps runs each. The
added milliseconds stand next to their floor: (requests with a non-zero tier)
x N x 8 bytes at the 8 TB/s HBM peak; their ratio is the HBM fraction of the
impact pass alone. One JSON file under profiles/whatif_impact/ (and the same
line on stdout)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from openr_amd import host_backend  # noqa: E402
from openr_amd.facade import load_topology  # noqa: E402
from openr_amd.types import K_TESTING_AREA as A  # noqa: E402
from openr_amd.workloads import (C4_WHATIF_CHUNK, c4_drain_job, c4_node_weights, c4_wan,  # noqa: E402
                                 c4_what_if_job)

HBM_PEAK = 8e12  # bytes / s


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3), "runs_ms": [round(x, 3) for x in ms]}


def top(rec, field, srcs, idx, what, names, k=10):
    order = np.argsort(-rec[field].astype(np.float64), kind="stable")[:k]
    out = []
    for i in order:
        i = int(i)
        wn = int(rec["worst_node"][i])
        out.append({"request": i, "source": srcs[idx[i]], "what": what[i], field: int(rec[field][i]),
                    "lost": int(rec["lost"][i]), "farther": int(rec["farther"][i]),
                    "rehomed": int(rec["rehomed"][i]), "narrowed": int(rec["narrowed"][i]),
                    "max_stretch": int(rec["max_stretch"][i]),
                    "worst_node": names[wn] if wn != 0xFFFFFFFF else None})
    return out


def measure(job, weights, reps, n_nodes, srcs, idx, what, names):
    def once(on):
        job.set_impact(on, weights if on else None, node_counts=on)
        job.run()
        job.sync()
        return job.last_ms()
    once(False), once(True)  # warm-up of both forms
    off, on = [], []
    for _ in range(reps):
        off.append(once(False))
        on.append(once(True))
    rec = job.impact()
    lost, moved = job.node_impact()
    tier = job.info() & 7
    scanned = int(np.sum(tier != 0))
    added = statistics.median(on) - statistics.median(off)
    floor = scanned * n_nodes * 8 / HBM_PEAK * 1e3
    out = {"requests": len(idx), "scanned_requests": scanned, "off": spread(off), "on": spread(on),
           "added_ms": round(added, 3), "floor_ms_at_8TBps": round(floor, 3),
           "hbm_fraction_of_impact_pass": round(floor / added, 3) if added > 0 else None,
           "requests_with_lost": int(np.sum(rec["lost"] > 0)),
           "requests_with_farther": int(np.sum(rec["farther"] > 0)),
           "requests_with_rehomed": int(np.sum(rec["rehomed"] > 0)),
           "max_stretch": int(rec["max_stretch"].max()),
           "nodes_ever_lost": int(np.sum(lost > 0)), "nodes_ever_moved": int(np.sum(moved > 0)),
           "top_lost_weight": top(rec, "lost_weight", srcs, idx, what, names),
           "top_moved_weight": top(rec, "moved_weight", srcs, idx, what, names)}
    job.release()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=4096, help="links / drained nodes of the jobs")
    ap.add_argument("--srcs", type=int, default=64)
    ap.add_argument("--chunk", type=int, default=C4_WHATIF_CHUNK)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "whatif_impact", "c4_impact.json"))
    args = ap.parse_args()
    if args.reps < 5:
        ap.error("--reps must be at least 5")

    hip = host_backend()
    adj, _ = c4_wan()
    als, _ = load_topology(hip, adj, [])
    ls = als[A]._impl
    names = ls.node_names()
    weights = c4_node_weights(names)
    out = {"tool": "whatif_impact", "graph_nodes": len(names), "chunk": args.chunk, "reps": args.reps}

    links = dict(ls.link_ids())
    srcs, idx, sets = c4_what_if_job(list(links), names, args.nodes, args.srcs)
    what = ["link %s-%s" % (links[s[0]][0], links[s[0]][2]) for s in sets]
    job = ls.what_if_batch(srcs, idx, sets, args.chunk)
    out["link_job"] = measure(job, weights, args.reps, len(names), srcs, idx, what, names)
    del job
    srcs, idx, ignore, drain = c4_drain_job(names, args.nodes, args.srcs)
    what = ["drain %s" % d[0] for d in drain]
    job = ls.what_if_batch(srcs, idx, ignore, args.chunk, drain=drain)
    out["drain_job"] = measure(job, weights, args.reps, len(names), srcs, idx, what, names)
    del job
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
