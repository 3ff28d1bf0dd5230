"""A/B of one all-sources sweep alone on the device under environment specs
that the graph load reads (ORH_MS_ADJ, ORH_MS_ORDER, ORH_MS_SKIP, ...), per
topology, the specs alternating in one process, each on a fresh device mirror:
median and minimum device ms of the sweeps and the median per phase
[search + finalize, first hops]. Last lines: what each graph takes with none
of the specs set.

  ORH_BFS_NH_MAX=0 python tools/ms_env_ab.py --specs ORH_MS_ADJ=0 ORH_MS_ADJ=1 \
      --topos c3,c5a,grid25,grid70 [--rounds 2] [--reps 20]

Topologies: c3 (the 2,472-node Clos), c5a (area A of the C5 graph), gridS.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from openr_amd import host_backend  # noqa: E402
from openr_amd.facade import load_topology  # noqa: E402
from openr_amd.topology import bench_grid  # noqa: E402
from openr_amd.types import K_TESTING_AREA  # noqa: E402


def topology(name):
    if name == "c3":
        from openr_amd.workloads import c3_fabric
        return "c3_fabric", c3_fabric(num_prefixes=0)[0], K_TESTING_AREA
    if name == "c5a":
        from openr_amd.workloads import c5_multi_area
        return "c5_area_A", c5_multi_area(num_prefixes=0)[0]["A"], "A"
    if name.startswith("grid"):
        return name, bench_grid(int(name[4:]))[0], K_TESTING_AREA
    raise SystemExit(f"unknown topology {name!r}")


def sweep_ms(hip, dbs, area, reps):
    als, _ = load_topology(hip, dbs, [])
    ls = als[area]._impl
    names = [db.thisNodeName for db in dbs]
    sw = ls.sweep(names, True)
    tot, dist, hop = [], [], []
    for _ in range(reps + 1):
        sw.run()
        sw.sync()
        d, h = sw.phase_ms()
        tot.append(d + h)
        dist.append(d)
        hop.append(h)
    return ls.ms_order()[0], sw.info(), tot[1:], dist[1:], hop[1:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--specs", nargs="+", required=True, help="VAR=value[,VAR=value] per spec")
    ap.add_argument("--topos", default="c3,c5a,grid25,grid70")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    hip = host_backend()
    touched = sorted({kv.split("=")[0] for s in args.specs for kv in s.split(",")})
    defaults = []
    for t in args.topos.split(","):
        name, dbs, area = topology(t)
        for _ in range(args.rounds):
            for spec in args.specs:
                for k in touched:
                    os.environ.pop(k, None)
                for kv in spec.split(","):
                    k, v = kv.split("=")
                    os.environ[k] = v
                order, info, tot, dist, hop = sweep_ms(hip, dbs, area, args.reps)
                print(f"{name} {len(dbs)} {spec} order {order} variant {info['variant']} threads {info['ms_threads']} "
                      f"ms_adj {info['ms_adj']} ms_skip {info['ms_skip']} ms {statistics.median(tot):.4f} "
                      f"min {min(tot):.4f} phases [{statistics.median(dist):.4f}, {statistics.median(hop):.4f}]",
                      flush=True)
        for k in touched:
            os.environ.pop(k, None)
        order, info, _, _, _ = sweep_ms(hip, dbs, area, 1)
        defaults.append(f"{name} default: order {order} ms_adj {info['ms_adj']} ms_skip {info['ms_skip']}")
    print("\n".join(defaults))


if __name__ == "__main__":
    main()
