#!/usr/bin/env python3
"""C3w A/B: the all-sources sweep of the weighted Clos
(workloads.c3_weighted_fabric, N = 2,472, metrics 1..64) on the sliced
multi-source plan (ORH_WMS_SLICED=1, spf_wms_sliced_kernel) against the
two-phase per-source plan it replaces (ORH_WMS_SLICED=0), alternating in one
process: --reps sweeps each after a warm-up of both. Per plan: median / min /
max device ms of a sweep (HIP events: distances + first hops), the median
phase split, the plan's info; the layout's padded-to-real slot ratio; and
every row of both plans against the fast checker's rows by row digest.
--all-c2w-deg: the same A/B under ORH_WMS_SLICED_ALL=1 on a random weighted
graph of --n nodes with 9..32 neighbours each, against the fused LDS search
(kLdsNh) that such sweeps take by default; --check-rows seeded rows of it are
checked. One JSON line."""
import argparse
import json
import os
import random
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "build"))


def degree_graph(n, seed, max_metric=64):
    """Connected random graph, every node with 9..32 distinct neighbours,
    one seeded metric per link (both directions)."""
    from openr_amd.types import K_TESTING_AREA, Adjacency, BinaryAddress, create_adj_db
    rng = random.Random(seed)
    nbrs = [set() for _ in range(n)]
    adjs = [[] for _ in range(n)]
    v6, v4 = BinaryAddress.of("fe80::1"), BinaryAddress.of("10.0.0.1")

    def link(a, b):
        if a == b or b in nbrs[a] or len(nbrs[a]) >= 32 or len(nbrs[b]) >= 32:
            return
        w = rng.randint(1, max_metric)
        nbrs[a].add(b)
        nbrs[b].add(a)
        for x, y in ((a, b), (b, a)):
            adjs[x].append(Adjacency(f"n{y}", f"n{x}-n{y}", v6, v4, w, 0, False, 0, 0, 1, f"n{y}-n{x}"))

    for i in range(n):
        link(i, (i + 1) % n)
    for i in range(n):
        want = rng.randint(9, 32)
        for _ in range(200):
            if len(nbrs[i]) >= want:
                break
            # mostly near ids (a banded graph, as a fabric's layout would be), some far
            j = (i + rng.randint(2, 64)) % n if rng.random() < 0.8 else rng.randrange(n)
            link(i, j)
    assert min(len(s) for s in nbrs) >= 9, "degree floor not reached"
    return [create_adj_db(f"n{i}", adjs[i], i + 1, False, K_TESTING_AREA) for i in range(n)]


def ab(hip, oracle_mod, dbs, reps, check_rows, threads, knob="ORH_WMS_SLICED"):
    """The A/B of one per-run knob (1 against 0) on the all-sources sweep of dbs."""
    from helpers import row_digest
    from openr_amd.facade import Backend, load_topology
    from openr_amd.types import K_TESTING_AREA as A
    als, _ = load_topology(hip, dbs, [])
    ls = als[A]._impl
    names = [db.thisNodeName for db in dbs]
    sw = ls.sweep(names, True)
    plans = {"0": {"ms": [], "ph": []}, "1": {"ms": [], "ph": []}}
    for flag in ("0", "1"):  # warm-up: layouts, staging, kernel attributes
        os.environ[knob] = flag
        sw.run()
        sw.sync()
    for _ in range(reps):
        for flag in ("0", "1"):
            os.environ[knob] = flag
            sw.run()
            plans[flag]["ms"].append(sw.last_ms())
            plans[flag]["ph"].append(sw.phase_ms())
            plans[flag]["info"] = sw.info()
    # rows of both plans against the checker, by digest
    als_o, _ = load_topology(Backend(oracle_mod, "oracle"), dbs, [])
    order = ls.node_names()
    ids = {nm: i for i, nm in enumerate(order)}
    fc = oracle_mod.FastChecker(als_o[A]._impl, order)
    rows = list(range(len(names)))
    if check_rows and check_rows < len(rows):
        rows = sorted(random.Random(5).sample(rows, check_rows))
    out = {}
    for flag in ("0", "1"):
        os.environ[knob] = flag
        sw.run()
        sw.sync()
        bad = 0
        for lo in range(0, len(rows), 512):
            part = rows[lo:lo + 512]
            dist, nh = fc.spf_rows([ids[names[i]] for i in part], [], threads)
            w = min(sw.words, nh.shape[2])
            for k, i in enumerate(part):
                d, m = sw.fetch(i)
                m = m.reshape(-1, sw.words)
                if m[:, w:].any() or nh[k][:, w:].any() or row_digest(d, m[:, :w]) != row_digest(dist[k], nh[k][:, :w]):
                    bad += 1
        p = plans[flag]
        out["sliced" if flag == "1" else "off"] = {
            "device_ms": {"median": round(statistics.median(p["ms"]), 4), "min": round(min(p["ms"]), 4),
                          "max": round(max(p["ms"]), 4)},
            "phase_ms": [round(statistics.median(x[i] for x in p["ph"]), 4) for i in (0, 1)],
            "info": p["info"], "rows_checked": len(rows), "digest_mismatches": bad}
    os.environ.pop(knob, None)
    si = out["sliced"]["info"]
    out["nodes"], out["sources"], out["reps"] = sw.nodes, len(names), reps
    out["padded_to_real_slots"] = round(si["wsl_slots"] / si["wsl_links"], 3) if si.get("wsl_links") else None
    a, b = out["sliced"]["device_ms"], out["off"]["device_ms"]
    out["sliced_faster_disjoint"] = a["median"] < b["median"] and a["max"] < b["min"]
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--nodes", type=int, default=2500, help="fabric size (2,472 nodes at 2,500)")
    p.add_argument("--all-c2w-deg", action="store_true")
    p.add_argument("--n", type=int, default=10_000, help="--all-c2w-deg: nodes of the random graph")
    p.add_argument("--check-rows", type=int, default=500, help="--all-c2w-deg: rows checked (0: all)")
    p.add_argument("--threads", type=int, default=16)
    args = p.parse_args()
    import importlib
    from openr_amd import host_backend
    from openr_amd.workloads import c3_weighted_fabric
    hip = host_backend()
    oracle_mod = importlib.import_module("openr_oracle")
    dbs, _ = c3_weighted_fabric(args.nodes)
    out = {"c3w": ab(hip, oracle_mod, dbs, max(args.reps, 7), 0, args.threads)}
    if args.all_c2w_deg:
        os.environ["ORH_WMS_SLICED_ALL"] = "1"
        out["c2w_deg"] = ab(hip, oracle_mod, degree_graph(args.n, 77), max(args.reps, 7), args.check_rows,
                            args.threads)
        os.environ.pop("ORH_WMS_SLICED_ALL", None)
    out["env"] = {k: v for k, v in os.environ.items() if k.startswith("ORH_")}
    print(json.dumps(out), flush=True)
    ok = all(v[k]["digest_mismatches"] == 0 for v in out.values() if isinstance(v, dict) and "sliced" in v
             for k in ("sliced", "off"))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
