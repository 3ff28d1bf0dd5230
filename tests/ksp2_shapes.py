"""Topologies at the bounds of the KSP2 device traces (ksp_kernels.hip), with
the (device, host) split each trace kernel must give, derived from the caps in
the code (test_gpu_ksp2_edges.py states the derivations).

Every shape is a dict: ``dbs`` (adjacency databases in load order), ``pairs``
(one prefetchKthPaths batch, bound pairs between short ones), and the pairs
each kernel must flag for the host: ``host_wave`` (ksp_trace_wave_kernel, the
default) and ``host_thread`` (ksp_trace_kernel, ORH_KSP_WAVE=0). Imported by
the tests and by their child processes (one per process-wide switch).
"""
from openr_amd.types import Adjacency, BinaryAddress, create_adj_db

# api/ksp.hip (orh_ksp2_batch) and ksp_kernels.hip
OUT_CAP, IGN_CAP = 1024, 512
WAVE_STACK, WAVE_HASH = 512, 1024
THREAD_STACK, THREAD_HASH = 1024, 2048

_NH6, _NH4 = BinaryAddress.of("fe80::1"), BinaryAddress.of("10.0.0.1")


def build(links, overloaded=()):
    """links: (a, b, metric a->b, metric b->a), parallel ones repeated; a
    node's adjacencies (and the databases) in first-appearance order."""
    adjs, count = {}, {}
    for a, b, m_ab, m_ba in links:
        k = count.get((a, b), 0)
        count[(a, b)] = count[(b, a)] = k + 1
        adjs.setdefault(a, []).append(Adjacency(b, f"{a}>{b}#{k}", _NH6, _NH4, m_ab, 0, False, 0, 0, 1,
                                                f"{b}>{a}#{k}"))
        adjs.setdefault(b, []).append(Adjacency(a, f"{b}>{a}#{k}", _NH6, _NH4, m_ba, 0, False, 0, 0, 1,
                                                f"{a}>{b}#{k}"))
    return [create_adj_db(n, a, 0, n in overloaded) for n, a in adjs.items()]


def ell_width(dbs):
    """The loader's rule (choose_ell_k): 8 when the node degree at the ninth
    decile is above 4, else 4; a node's degree is its number of links."""
    deg = sorted(len(db.adjacencies) for db in dbs)
    return 8 if deg[len(deg) * 9 // 10] > 4 else 4


def _both(pairs):
    return {p for s, d in pairs for p in ((s, d), (d, s))}


def path_graph():
    n = 520
    dbs = build([(f"p{i}", f"p{i + 1}", 1, 1) for i in range(n - 1)])
    pairs = [("p3", "p9"), ("p0", "p511"), ("p0", "p512"), ("p0", "p513"), ("p10", "p4"), ("p513", "p0"),
             ("p512", "p0"), ("p511", "p0"), ("p519", "p500"), ("p0", "p1")]
    return dict(dbs=dbs, pairs=pairs, host_wave=_both([("p0", "p512"), ("p0", "p513")]),
                host_thread=_both([("p0", "p513")]))


def ring():
    n = 612
    dbs = build([(f"r{i}", f"r{(i + 1) % n}", 1, 1) for i in range(n)])
    # a pair d links apart has k = 2 the other way round, 612 - d links: the
    # neighbours in batch order are 101..305 apart so that the device keeps them
    pairs = [("r5", "r150"), ("r0", "r101"), ("r0", "r100"), ("r400", "r200"), ("r0", "r306"), ("r0", "r256"),
             ("r300", "r150"), ("r100", "r0"), ("r101", "r0"), ("r0", "r1")]
    return dict(dbs=dbs, pairs=pairs,
                host_wave={("r0", "r100"), ("r100", "r0"), ("r0", "r306"), ("r0", "r1")},
                host_thread={("r0", "r306")})


def two_rings():
    """Rings of 512 and of 514 nodes: the antipodal pair has two k = 1 paths
    of 256 / 257 links, 512 / 514 links in all."""
    links = [(f"{r}{i}", f"{r}{(i + 1) % n}", 1, 1) for r, n in (("u", 512), ("v", 514)) for i in range(n)]
    pairs = [("u7", "u2"), ("u0", "u256"), ("u300", "u301"), ("v0", "v257"), ("v9", "v4"), ("v257", "v0"),
             ("u256", "u0"), ("v1", "v0")]
    return dict(dbs=build(links), pairs=pairs,
                host_wave=_both([("u0", "u256"), ("v0", "v257")]) | {("v1", "v0")},
                host_thread=_both([("v0", "v257")]))


def theta(length):
    """S - T by one link, and by two ways a, b of `length` links each: k = 1
    is the link, k = 2 the two ways."""
    a = ["s"] + [f"a{i}" for i in range(1, length)] + ["t"]
    b = ["s"] + [f"b{i}" for i in range(1, length)] + ["t"]
    links = [("s", "t", 1, 1)] + [(w[i], w[i + 1], 1, 1) for w in (a, b) for i in range(length)]
    pairs = [("a3", "a9"), ("s", "t"), ("b20", "b12"), ("t", "s"), ("a1", "s")]
    flagged = _both([("s", "t")])
    return dict(dbs=build(links), pairs=pairs, host_wave=flagged, host_thread=flagged if length > 507 else set())


FAN_SIZES = (255, 256, 257)


def fans():
    """Three fans in one graph (one component each): S - m_i - T for M mids,
    and the detour S - x - y - T (3 links against 2) for k = 2."""
    links = []
    for m in FAN_SIZES:
        s, t = f"f{m}s", f"f{m}t"
        for i in range(m):
            links += [(s, f"f{m}m{i}", 1, 1), (f"f{m}m{i}", t, 1, 1)]
        links += [(s, f"f{m}x", 1, 1), (f"f{m}x", f"f{m}y", 1, 1), (f"f{m}y", t, 1, 1)]
    pairs = [("f255m1", "f255m2"), ("f255s", "f255t"), ("f255t", "f255s"), ("f256m1", "f256m2"),
             ("f256s", "f256t"), ("f256m5", "f256s"), ("f256t", "f256s"), ("f257s", "f257t"),
             ("f257m0", "f257m3"), ("f257t", "f257s"), ("f255m7", "f255t"), ("f255x", "f255t"),
             ("f256x", "f256t"), ("f257m9", "f257s")]
    return dict(dbs=build(links), pairs=pairs,
                host_wave=_both([("f256s", "f256t"), ("f257s", "f257t")]) | {("f256x", "f256t"), ("f257m9", "f257s")},
                host_thread=_both([("f257s", "f257t")]))


def big_fans():
    """Fans of 511 and 512 mids with the detour S - x - y - T; only pairs whose
    traces meet the mids on failing branches (k = 2 of (x, T) and of (y, S)
    consumes 2 M + 1 links), none that finds M paths."""
    links = []
    for m in (511, 512):
        s, t = f"g{m}s", f"g{m}t"
        for i in range(m):
            links += [(s, f"g{m}m{i}", 1, 1), (f"g{m}m{i}", t, 1, 1)]
        links += [(s, f"g{m}x", 1, 1), (f"g{m}x", f"g{m}y", 1, 1), (f"g{m}y", t, 1, 1)]
    pairs = [("g511m1", "g511m2"), ("g511x", "g511t"), ("g512m3", "g512m4"), ("g512x", "g512t"),
             ("g511x", "g511y"), ("g511y", "g511s"), ("g512m7", "g512m9"), ("g512y", "g512s"), ("g512y", "g512x")]
    flagged = {("g511x", "g511t"), ("g511y", "g511s"), ("g512x", "g512t"), ("g512y", "g512s")}
    return dict(dbs=build(links), pairs=pairs, host_wave=flagged,
                host_thread={("g512x", "g512t"), ("g512y", "g512s")})


# (name, parallel links, with the two-link detour)
BUNDLES = (("a", 508, True), ("b", 509, True), ("c", 510, False), ("d", 511, False))


def parallel_bundles():
    """M parallel links S - T of metric 1 per bundle (one component each), a
    pendant u on S for the short pairs, and for two of them the detour
    S - x - T of two links."""
    links, pairs = [], []
    for name, m, detour in BUNDLES:
        s, t, u = f"{name}s", f"{name}t", f"{name}u"
        links += [(s, t, 1, 1)] * m + [(s, u, 1, 1)]
        if detour:
            links += [(s, f"{name}x", 1, 1), (f"{name}x", t, 1, 1)]
        pairs += [(u, s), (s, t), (s, u), (t, s), (u, t)]
    flagged = _both([("bs", "bt"), ("ds", "dt")])
    return dict(dbs=build(links), pairs=pairs, host_wave=flagged | {("du", "dt")}, host_thread=flagged)


def _padding(kind, at):
    """ell 4: 30 pendant leaves on `at`; ell 8: a clique of 12 hung on `at`."""
    if kind == 4:
        return [(at, f"leaf{i}", 1, 1) for i in range(30)]
    c = [f"c{i:02d}" for i in range(12)]
    return [(c[i], c[j], 1, 1) for i in range(12) for j in range(i + 1, 12)] + [(at, c[0], 1, 1)]


def bundles70(kind):
    """S = 70 links = P = 70 links = T; the metrics differ by direction and
    tie inside a bundle."""
    links = [("S", "P", 3, 5)] * 70 + [("P", "T", 2, 7)] * 70 + _padding(kind, "P")
    far = "leaf7" if kind == 4 else "c05"
    pairs = [("S", "P"), ("S", "T"), (far, "T"), ("T", "S"), ("P", "T"), ("T", far), (far, "S")]
    return dict(dbs=build(links), pairs=pairs, host_wave=set(), host_thread=set())


def hub80(kind):
    """A hub with 80 spokes and a few chords that tie with the way through
    the hub (metric 2 against 1 + 1) or beat it (metric 1)."""
    links = [("hub", f"l{i:02d}", 1, 1) for i in range(80)]
    links += [("l00", "l01", 2, 2), ("l10", "l50", 2, 2), ("l03", "l04", 1, 1), ("l04", "l05", 1, 1),
              ("l70", "l79", 2, 1), ("l70", "l79", 2, 1), ("l20", "l60", 3, 3)]
    links += _padding(kind, "hub")
    far = "leaf3" if kind == 4 else "c07"
    pairs = [("l05", "l60"), ("l00", "l01"), ("l10", "l50"), ("l79", "l02"), ("l03", "l05"), ("l70", "l79"),
             ("l79", "l70"), (far, "l33"), ("l20", "l60"), ("l44", far), ("hub", "l04"), ("l04", "hub")]
    return dict(dbs=build(links), pairs=pairs, host_wave=set(), host_thread=set())


def defects():
    """A chain a - b - c - d - e with b overloaded (no transit), a second way
    a - g - h - e through the overloaded h only, and a component x - y - z."""
    links = [("a", "b", 1, 1), ("b", "c", 1, 1), ("c", "d", 1, 1), ("d", "e", 1, 1), ("a", "g", 1, 1),
             ("g", "h", 1, 1), ("h", "e", 1, 1), ("x", "y", 1, 1), ("y", "z", 1, 1), ("x", "z", 2, 2)]
    pairs = [("a", "a"), ("a", "c"), ("a", "x"), ("b", "e"), ("a", "b"), ("x", "z"), ("z", "a"), ("e", "c"),
             ("a", "h"), ("g", "e"), ("b", "b"), ("h", "a")]
    empty = {("a", "a"), ("a", "c"), ("a", "x"), ("z", "a"), ("b", "b"), ("g", "e")}
    return dict(dbs=build(links, overloaded=("b", "h")), pairs=pairs, host_wave=set(), host_thread=set(),
                empty=empty)


def random_all_pairs():
    from test_gpu_parity import random_topology
    dbs = random_topology(2100, n=20, extra=34, max_metric=4, parallel=0.4, overload=0.1, link_overload=0.06)
    names = sorted(db.thisNodeName for db in dbs)
    return dict(dbs=dbs, pairs=[(s, d) for s in names for d in names], host_wave=set(), host_thread=set())


SHAPES = {
    "path": path_graph,
    "ring": ring,
    "two_rings": two_rings,
    "theta507": lambda: theta(507),
    "theta508": lambda: theta(508),
    "fans": fans,
    "big_fans": big_fans,
    "parallel": parallel_bundles,
    "bundles70_ell4": lambda: bundles70(4),
    "bundles70_ell8": lambda: bundles70(8),
    "hub80_ell4": lambda: hub80(4),
    "hub80_ell8": lambda: hub80(8),
    "defects": defects,
    "random": random_all_pairs,
}
