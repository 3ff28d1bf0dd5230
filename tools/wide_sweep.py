#!/usr/bin/env python3
"""Wide-label A/B: all-sources weighted sweeps whose metrics or distances pass
16 bits, on the wide multi-source plan (spf_wms_wide_kernel) against what the
sweep runs without it, alternating in one process (c3w_sweep.ab: --reps sweeps
each after a warm-up of both, device ms from HIP events, the phase split, the
plan's info, every row of both plans against the fast checker by row digest).

  c3w_x1000  workloads.c3_weighted_fabric() with every metric x 1,000
             (N = 2,472, metrics up to 64,000): ORH_WMS_WIDE=1 (kWmsWide)
             against 0 (the two-phase per-source plan)
  c2w_60k    workloads.c2_weighted_grid(100, max_metric=60_000) (N = 10,000):
             ORH_WMS_WIDE=1 against 0 (spf_lds_nh_kernel)
  clos_20k   the Clos at metrics 19,990..20,000 (every row of the sliced u16
             plan is flagged): ORH_WMS_WIDE_REDO=1 (flagged rows redone in wide
             batches) against 0 (redone per source)

One JSON line per shape; --shapes picks among them."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "build"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

SHAPES = ("c3w_x1000", "c2w_60k", "clos_20k")


def workload(shape, nodes):
    """(adjacency databases, the knob of the A/B)."""
    from openr_amd.topology import fabric
    from openr_amd.workloads import c2_weighted_grid, c3_weighted_fabric, weight_links
    if shape == "c3w_x1000":
        dbs, _ = c3_weighted_fabric(nodes)
        for db in dbs:
            for adj in db.adjacencies:
                adj.metric *= 1000
        return dbs, "ORH_WMS_WIDE"
    if shape == "c2w_60k":
        return c2_weighted_grid(100, max_metric=60_000)[0], "ORH_WMS_WIDE"
    dbs, _ = fabric(nodes, bug_compatible=False)
    return weight_links(dbs, 19_990, 20_000, 10, True), "ORH_WMS_WIDE_REDO"


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--nodes", type=int, default=2500, help="fabric size (2,472 nodes at 2,500)")
    p.add_argument("--shapes", default=",".join(SHAPES))
    p.add_argument("--check-rows", type=int, default=0, help="rows checked per plan (0: all)")
    p.add_argument("--threads", type=int, default=16)
    args = p.parse_args()
    from c3w_sweep import ab
    from openr_amd import host_backend
    hip = host_backend()
    oracle_mod = importlib.import_module("openr_oracle")
    ok = True
    for shape in args.shapes.split(","):
        dbs, knob = workload(shape, args.nodes)
        r = ab(hip, oracle_mod, dbs, max(args.reps, 7), args.check_rows, args.threads, knob=knob)
        r["on"] = r.pop("sliced")
        r["on_faster_disjoint"] = r.pop("sliced_faster_disjoint")
        r.update(shape=shape, knob=knob, env={k: v for k, v in os.environ.items() if k.startswith("ORH_")})
        print(json.dumps(r), flush=True)
        ok = ok and r["on"]["digest_mismatches"] == 0 and r["off"]["digest_mismatches"] == 0
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
