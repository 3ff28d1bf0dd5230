"""The route kernels at the C boundary (``-m gpu``): route_select_kernel,
route_diff_kernel, route_policy_kernel, scatter_hdr_kernel and the prefix
mirror, driven through orh_route_select* / orh_route_diff / orh_route_policy*
/ orh_prefix_* with ctypes and compared, array for array and exactly, with
the plain model of tests/route_model.py (itself pinned to the oracle in
tests/test_route_model.py).

No SPF runs: dist / nh / overloaded / name_node are synthetic seeded arrays
of 40-70 nodes per area, since the kernels are functions of those arrays and
arbitrary rows reach states a real topology rarely does (a name that is
nearer in an area it is not advertised in, all-drained sets, rows without a
first hop, ...). Output buffers start as 0xA5 bytes, so an entry the kernel
did not write, or wrote outside its range, shows.

What is compared: status, metric and every mask word of every prefix (the
header fixes metric = ORH_UNREACHABLE and a zero mask for NONE / HOST);
best[p] for ROUTE, and for the rest only that it was written and is below
the list's length, which is all the header promises.
"""
import ctypes
import random

import numpy as np
import pytest

import route_abi as ra
import route_model as rm

pytestmark = pytest.mark.gpu

I32_MAX, I32_MIN = (1 << 31) - 1, -(1 << 31)
ALL_FLAGS = (0, rm.SELECT_BEST_ROUTE, rm.SELECT_V4, rm.SELECT_BEST_ROUTE | rm.SELECT_V4)
N_TAGSETS = 6


@pytest.fixture(scope="module")
def dev():
    from openr_amd import HIP_LIB_PATH
    d = ra.Device(ctypes.CDLL(HIP_LIB_PATH))  # as built; a missing library is an error
    yield d
    d.close()


# ---- generators ---------------------------------------------------------------

def make_areas(rng, n_names, words, offsets, me, absent=0.1, second=0.3):
    """Synthetic areas: every name gets a home area (except `absent` of them)
    and with probability `second` one more; about 20 % of the nodes are
    unreachable, 20 % overloaded, some reachable rows have no first hop.
    `me` is a node of every area at distance 0."""
    n_areas = len(words)
    member = [[] for _ in range(n_areas)]
    for name in range(n_names):
        if name != me and rng.random() < absent:
            continue
        home = rng.randrange(n_areas)
        member[home].append(name)
        if name == me:
            for b in range(n_areas):
                if b != home:
                    member[b].append(name)
        elif n_areas > 1 and rng.random() < second:
            member[rng.choice([b for b in range(n_areas) if b != home])].append(name)
    areas = []
    for b in range(n_areas):
        N = max(40, min(70, len(member[b]) + rng.randint(2, 8)), len(member[b]))
        ids = rng.sample(range(N), len(member[b]))
        name_node = np.full(n_names, rm.NO_NODE, np.uint32)
        for name, v in zip(member[b], ids):
            name_node[name] = v
        dist = np.array([rm.UNREACHABLE if rng.random() < 0.2 else rng.randint(1, 12) for _ in range(N)], np.uint32)
        nh = np.zeros((N, words[b]), np.uint32)
        for v in range(N):
            if dist[v] != rm.UNREACHABLE and rng.random() < 0.92:
                for w in range(words[b]):
                    nh[v, w] = rng.getrandbits(32) & rng.getrandbits(32) & rng.getrandbits(32)
                if rng.random() < 0.3:
                    nh[v, rng.randrange(words[b])] |= 1 << rng.choice((0, 31))
        ovl = np.array([rng.random() < 0.2 for _ in range(N)], np.uint8)
        dist[name_node[me]], nh[name_node[me]] = 0, 0
        areas.append(dict(present=1, dist=dist, nh=nh, ovl=ovl, name_node=name_node, words=words[b],
                          word_off=offsets[b]))
    return areas


def rand_prefix(rng, areas, n_names, me, max_adv=6):
    """One prefix of the fuzz: 0-6 advertisements with distinct (name, area)."""
    n_areas = len(areas)
    r = rng.random()
    cnt = 0 if r < 0.04 else rng.randint(1, max_adv)
    pflags = rm.PFX_V4 if rng.random() < 0.05 else 0
    special = rng.random()
    kind = None
    for k, name in enumerate(("bgp", "sr", "ksp2", "minnh", "self", "area")):
        if special < 0.04 * (k + 1):
            kind = name
            break
    pairs, advs = set(), []
    while len(pairs) < cnt:
        x = rng.random()
        if x < 0.03:
            name = n_names + rng.randrange(4)  # no such name
        else:
            name = rng.randrange(n_names)
            if name == me:
                continue
        homes = [b for b in range(n_areas) if name < n_names and areas[b]["name_node"][name] != rm.NO_NODE]
        area = rng.choice(homes) if homes and rng.random() < 0.85 else rng.randrange(n_areas)
        pairs.add((name, area))
    everyone = rng.random() < 0.5
    for k, (name, area) in enumerate(sorted(pairs, key=lambda _: rng.random())):
        meta = area
        mark = everyone or k == 0
        if kind == "bgp" and mark:
            meta |= rm.ADV_BGP
        if kind == "sr" and mark:
            meta |= rm.ADV_SR_MPLS
        if kind == "ksp2" and mark:
            meta |= rm.ADV_KSP2
        if kind == "minnh" and mark:
            meta |= rm.ADV_MIN_NEXTHOP
        if kind == "area" and k == 0:
            meta = n_areas + rng.randrange(3)
        if rng.random() < 0.1:
            meta |= rm.ADV_PREPEND
        ts = rng.choice((0, 0, 1, 2, 3, 4, N_TAGSETS - 1, N_TAGSETS, N_TAGSETS + 3, rm.TAGSET_OVF))
        meta |= ts << rm.TAGSET_SHIFT
        d = rng.choice((0, 0, 1, 1, 2, -1, I32_MAX, I32_MIN))
        advs.append((name, meta, rng.randint(-2, 2), rng.randint(-2, 2), d))
    if kind == "self" and advs:
        advs.insert(rng.randrange(len(advs) + 1), (me, rng.randrange(n_areas), 0, 0, 0))
    return (pflags, advs)


WORDS = {1: [(1,), (2,), (3,)], 3: [(2, 3, 1), (3, 1, 2), (3, 3, 1)]}
OFFSET_ORDER = {1: (0,), 3: (2, 0, 1)}  # word_off is not in area order


def fuzz_case(seed, n_prefix, n_areas):
    rng = random.Random(seed * 7919 + n_prefix * 31 + n_areas)
    words = WORDS[n_areas][seed % 3]
    offsets, at = [0] * n_areas, 0
    for b in OFFSET_ORDER[n_areas]:
        offsets[b] = at
        at += words[b]
    n_names = 60 if n_areas == 1 else 110
    me = rng.randrange(n_names)
    areas = make_areas(rng, n_names, words, offsets, me)
    prefixes = [rand_prefix(rng, areas, n_names, me) for _ in range(n_prefix)]
    return dict(prefixes=prefixes, areas=areas, me=me, n_names=n_names, total_words=at,
                name_rank=np.arange(n_names, dtype=np.uint32), area_rank=np.arange(n_areas, dtype=np.uint32))


def hand_area(dist, nh, ovl=None, name_node=None, words=1, word_off=0, present=1):
    """An area whose node ids are the name ids unless name_node says otherwise."""
    n = len(dist) if dist is not None else len(nh)
    return dict(present=present, dist=None if dist is None else np.asarray(dist, np.uint32),
                nh=np.asarray(nh, np.uint32).reshape(n, words),
                ovl=np.zeros(n, np.uint8) if ovl is None else np.asarray(ovl, np.uint8),
                name_node=np.arange(n, dtype=np.uint32) if name_node is None else np.asarray(name_node, np.uint32),
                words=words, word_off=word_off)


# ---- driver -----------------------------------------------------------------

class Loaded:
    """A prefix set on the device with its area table."""

    def __init__(self, dev, case, order=True):
        self.dev, self.case = dev, case
        self.ps = ra.PrefixSet(dev)
        dev.ok(self.ps.load(case["prefixes"]))
        if order:
            dev.ok(self.ps.set_order(case["name_rank"], case["area_rank"]))
        self.tab = dev.areas(case["areas"])
        self.n_areas = len(case["areas"])
        self.n = len(case["prefixes"])

    def select(self, flags, out=None, lo=None, hi=None):
        out = out or ra.Out(self.dev, self.n, self.case["total_words"])
        self.dev.ok(self.ps.select(self.case["me"], flags, self.tab, self.n_areas, out, lo, hi))
        return out

    def model(self, flags):
        c = self.case
        return rm.select(c["prefixes"], c["areas"], c["me"], flags, c["name_rank"], c["area_rank"],
                         c["total_words"])

    def close(self):
        self.ps.close()
        self.dev.free_areas(self.tab, self.n_areas)


def assert_selection(got, want, prefixes, where=""):
    gs, gm, gb, gk = got
    ws, wm, wb, wk = want
    assert np.array_equal(gs, ws), (where, "status", np.nonzero(gs != ws)[0][:8])
    assert np.array_equal(gm, wm), (where, "metric", np.nonzero(gm != wm)[0][:8])
    assert np.array_equal(gk, wk), (where, "mask", np.nonzero((gk != wk).any(axis=1))[0][:8])
    route = ws == rm.SEL_ROUTE
    assert np.array_equal(gb[route].astype(np.int64), wb[route]), (where, "best")
    cnt = np.array([max(len(a), 1) for _, a in prefixes], np.uint32)
    assert np.all(gb[~route] < cnt[~route]), (where, "best of a non-route")


def run_and_check(dev, case, flags_list=ALL_FLAGS, min_routes=None):
    L = Loaded(dev, case)
    try:
        for flags in flags_list:
            want = L.model(flags)
            if min_routes is not None:
                assert int((want[0] == rm.SEL_ROUTE).sum()) >= min_routes, flags
            out = L.select(flags)
            assert_selection(out.read(), want, case["prefixes"], f"flags={flags}")
            out.free()
    finally:
        L.close()


# ---- selection ------------------------------------------------------------------

@pytest.mark.parametrize("n_areas", [1, 3])
@pytest.mark.parametrize("n_prefix", [1, 255, 256, 257, 1025])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_select_fuzz(dev, seed, n_prefix, n_areas):
    case = fuzz_case(seed, n_prefix, n_areas)
    # the fuzz does not hide behind HOST / NONE: at least half of the prefixes
    # are routes (one lone prefix may be anything)
    L = Loaded(dev, case)
    try:
        for flags in ALL_FLAGS:
            want = L.model(flags)
            if n_prefix > 1:
                assert 2 * int((want[0] == rm.SEL_ROUTE).sum()) >= n_prefix, (flags, np.bincount(want[0]))
            out = L.select(flags)
            assert_selection(out.read(), want, case["prefixes"], f"flags={flags}")
            out.free()
    finally:
        L.close()


def _onehot96(v):
    return [(1 << (v % 32)) if v // 32 == w else 0 for w in range(3)]


def test_select_advertiser_count_edge(dev):
    """1, 63, 64 and 65 advertisers, all reachable, distinct names: 64 is
    decided on the device with bit 63 of the candidate sets live, 65 is HOST;
    a withdrawn prefix between them is NONE."""
    n_names, me = 70, 0
    dist = [5] * n_names
    dist[0] = 0
    nh = [_onehot96(v) for v in range(n_names)]
    nh[0] = [0, 0, 0]

    def lst(k, best_at=None, near_at=None):
        # names descend, so the last advertisement has the smallest name
        out = []
        for i in range(k):
            out.append((k + 1 - i, 0, 9 if i == best_at else 0, 0, 0))
        return out
    area = hand_area(dist, nh, words=3)
    near = 64 + 1 - 63  # the name at index 63 of a 64-list
    prefixes = [(0, lst(1)), (0, lst(63)), (0, lst(64, best_at=63)), (0, []), (0, lst(64)), (0, lst(65)),
                (0, lst(64, best_at=0))]
    case = dict(prefixes=prefixes, areas=[area], me=me, n_names=n_names, total_words=3,
                name_rank=np.arange(n_names, dtype=np.uint32), area_rank=np.zeros(1, np.uint32))
    L = Loaded(dev, case)
    try:
        for flags in ALL_FLAGS:
            got = L.select(flags).read()
            assert_selection(got, L.model(flags), prefixes, f"flags={flags}")
            assert list(got[0]) == [1, 1, 1, 0, 1, 2, 1]
            assert got[2][2] == 63 and got[2][4] == 63  # the smallest name is the last one
            if flags & rm.SELECT_BEST_ROUTE:  # index 63 is the unique best: its first hop alone
                assert list(got[3][2]) == _onehot96(near)
        # index 63 the unique argmin: its node is nearer than every other
        area["dist"][near] = 1
        L2 = Loaded(dev, case)
        for flags in ALL_FLAGS:
            got = L2.select(flags).read()
            assert_selection(got, L2.model(flags), prefixes, f"argmin flags={flags}")
            assert got[1][4] == 1 and list(got[3][4]) == _onehot96(near)
        L2.close()
    finally:
        L.close()


def test_select_drained_filter(dev):
    """maybeFilterDrainedNodes: an all-overloaded set is kept, overloaded
    members of a mixed set leave, the best advertisement stays where it was,
    and overload is read in the advertisement's own area."""
    me = 0
    #            n0 n1 n2 n3 n4 n5 n6
    d0, o0 = [0, 3, 5, 4, 6, 2, 9], [0, 1, 0, 1, 0, 1, 1]
    d1, o1 = [0, 8, 7, 4, 6, 9, 9], [0, 0, 1, 0, 0, 1, 1]
    a0 = hand_area(d0, [0, 1, 2, 4, 8, 16, 32], o0, word_off=0)
    a1 = hand_area(d1, [0, 64, 128, 256, 512, 1024, 2048], o1, word_off=1)
    P = lambda *pairs: (0, [(n, a, 0, 0, 0) for n, a in pairs])
    prefixes = [
        P((5, 0), (6, 0)),          # 0 every member overloaded: the set is kept
        P((1, 0), (2, 0)),          # 1 n1 is nearer but drained: n2 alone
        P((2, 0), (1, 0)),          # 2 the best one (n1) is drained: best still points at it
        P((3, 1), (4, 1)),          # 3 n3 is overloaded in area 0 only: it stays
        P((3, 0), (4, 0)),          # 4 ... and leaves here
        P((1, 1), (2, 1)),          # 5 n1 overloaded in area 0 only, n2 in area 1 only
        P((5, 0), (5, 1)),          # 6 overloaded in both
    ]
    case = dict(prefixes=prefixes, areas=[a0, a1], me=me, n_names=7, total_words=2,
                name_rank=np.arange(7, dtype=np.uint32), area_rank=np.arange(2, dtype=np.uint32))
    L = Loaded(dev, case)
    try:
        for flags in ALL_FLAGS:
            got = L.select(flags).read()
            assert_selection(got, L.model(flags), prefixes, f"flags={flags}")
            s, m, b, k = got
            assert list(s) == [1] * 7
            assert (m[0], list(k[0])) == (2, [16, 0])
            # n2 alone: 5 in area 0; area 1 has it at 7
            assert (m[1], list(k[1])) == (5, [2, 0])
            assert (m[2], b[2], list(k[2])) == (5, 1, [2, 0])
            assert (m[3], list(k[3])) == (4, [4, 256])   # n3 at 4 in both areas
            assert (m[4], list(k[4])) == (6, [8, 512])   # n4 alone, 6 in both areas
            assert (m[5], list(k[5])) == (3, [1, 0])     # n1 kept (not overloaded in area 1): nearest in area 0
            assert (m[6], list(k[6])) == (2, [16, 0])
    finally:
        L.close()


def test_select_cross_area_minimum(dev):
    me, INF = 0, rm.UNREACHABLE
    #       n0 n1  n2 n3 n4   n5 n6 n7
    d0 = [0, 10, 7, 3, INF, 5, 4, 6]
    d1 = [0, 12, 7, 3, 2, 5, 4, 6]
    d2 = [0, 4, 9, 3, INF, 5, 4, 6]
    a0 = hand_area(d0, [[0, 0], [1, 2], [4, 8], [0, 0], [0, 0], [16, 0], [0, 0], [3, 3]], words=2, word_off=1)
    a1 = hand_area(d1, [0, 32, 64, 0, 128, 256, 0, 0], words=1, word_off=0)
    a2 = hand_area(d2, [0, 512, 1024, 0, 0, 2048, 0, 4096], words=1, word_off=3)
    a3 = hand_area(None, [0] * 8, words=1, word_off=4)            # present, me is not in it
    a4 = hand_area(None, [0] * 8, words=1, word_off=5, present=0)  # not present
    a4["name_node"] = None
    P = lambda *pairs: (0, [(n, a, 0, 0, 0) for n, a in pairs])
    prefixes = [
        P((1, 0)),          # 0 advertised in area 0, nearer in area 2
        P((2, 0)),          # 1 equal minima in areas 0 and 1
        P((5, 3)),          # 2 its area has no row of me: unreachable
        P((5, 3), (5, 0)),  # 3 ... the other entry makes the route
        P((1, 4)),          # 4 area not present
        P((1, 7)),          # 5 area id >= n_areas
        P((3, 0)),          # 6 argmin rows have no first hop
        P((3, 0), (6, 2)),  # 7 ... in any area
        P((4, 1)),          # 8 reachable only in its own area
        P((4, 0)),          # 9 unreachable in its own area, reachable in area 1
        P((7, 0), (1, 2)),  # 10 minimum 4 from area 2 alone although n7 ties nowhere
    ]
    case = dict(prefixes=prefixes, areas=[a0, a1, a2, a3, a4], me=me, n_names=8, total_words=6,
                name_rank=np.arange(8, dtype=np.uint32), area_rank=np.arange(5, dtype=np.uint32))
    L = Loaded(dev, case)
    try:
        for flags in ALL_FLAGS:
            got = L.select(flags).read()
            assert_selection(got, L.model(flags), prefixes, f"flags={flags}")
            s, m, b, k = got
            assert list(s) == [1, 1, 0, 1, 2, 2, 0, 0, 1, 0, 1]
            assert (m[0], list(k[0])) == (4, [0, 0, 0, 512, 0, 0])
            assert (m[1], list(k[1])) == (7, [64, 4, 8, 0, 0, 0])
            assert (m[3], list(k[3])) == (5, [256, 16, 0, 2048, 0, 0])
            assert (m[8], list(k[8])) == (2, [128, 0, 0, 0, 0, 0])
            assert (m[10], list(k[10])) == (4, [0, 0, 0, 512, 0, 0])
    finally:
        L.close()


def test_select_area_limit_and_argument_errors(dev):
    rng = random.Random(32)
    n_names, me, n_areas = 40, 0, 32
    areas = make_areas(rng, n_names, [1] * n_areas, list(rng.sample(range(n_areas), n_areas)), me, second=0.9)
    prefixes = [rand_prefix(rng, areas, n_names, me) for _ in range(300)]
    case = dict(prefixes=prefixes, areas=areas, me=me, n_names=n_names, total_words=n_areas,
                name_rank=np.arange(n_names, dtype=np.uint32), area_rank=np.arange(n_areas, dtype=np.uint32))
    run_and_check(dev, case, min_routes=100)

    L = Loaded(dev, case)
    out = ra.Out(dev, L.n, n_areas)
    try:
        tab33 = (ra.orh_select_area * 33)()
        for b in range(33):
            ctypes.memmove(ctypes.byref(tab33[b]), ctypes.byref(L.tab[b % 32]), ctypes.sizeof(ra.orh_select_area))
        assert L.ps.select(me, 0, tab33, 33, out) == ra.E_UNSUPPORTED
        saved = L.tab[5].word_off
        L.tab[5].word_off = n_areas  # word_off + words > total_words
        assert L.ps.select(me, 0, L.tab, n_areas, out) == ra.E_INVALID
        L.tab[5].word_off = saved
        assert L.ps.select(me, 0, L.tab, n_areas, out, 0, L.n + 1) == ra.E_INVALID
        assert L.ps.select(me, 0, L.tab, n_areas, out, 7, 6) == ra.E_INVALID
        # nothing was launched by the rejected calls
        dev.ok(dev.lib.orh_sync(dev.ctx))
        assert all(np.all(a.view(np.uint8) == ra.FILL) for a in out.read())
        fresh = Loaded(dev, case, order=False)
        assert fresh.ps.select(me, 0, fresh.tab, n_areas, out) == ra.E_STATE
        fresh.close()
    finally:
        L.close()


def test_select_range(dev):
    case = fuzz_case(1, 600, 3)
    flags = rm.SELECT_BEST_ROUTE | rm.SELECT_V4
    L = Loaded(dev, case)
    try:
        full = L.select(flags).read()
        assert_selection(full, L.model(flags), case["prefixes"])
        for lo, hi in [(0, 1), (1, 256), (255, 257), (300, 300), (257, 600)]:
            got = L.select(flags, lo=lo, hi=hi).read()
            for g, f in zip(got, full):
                assert np.array_equal(g[lo:hi], f[lo:hi]), (lo, hi)
                assert np.all(g[:lo].view(np.uint8) == ra.FILL) and np.all(g[hi:].view(np.uint8) == ra.FILL), (lo, hi)
        assert L.ps.select(case["me"], flags, L.tab, L.n_areas, ra.Out(dev, 601, case["total_words"]), 0,
                           601) == ra.E_INVALID
    finally:
        L.close()


def test_select_best_node_area_order(dev):
    """bestNodeArea follows the rank tables, not the ids: reversed ranks, and
    one name advertised from two areas, where the area rank decides."""
    case = fuzz_case(2, 257, 3)
    n_names = case["n_names"]
    case["name_rank"] = np.arange(n_names, dtype=np.uint32)[::-1].copy()
    case["area_rank"] = np.array([2, 1, 0], np.uint32)
    both = [name for name in range(n_names) if name != case["me"] and all(
        A["name_node"][name] != rm.NO_NODE and A["dist"][A["name_node"][name]] != rm.UNREACHABLE
        for A in (case["areas"][0], case["areas"][2]))]
    assert both
    pinned = []
    for name in both[:4]:
        pinned.append(len(case["prefixes"]))
        case["prefixes"].append((0, [(name, 0, 1, 1, 0), (name, 2, 1, 1, 0)]))
        pinned.append(len(case["prefixes"]))
        case["prefixes"].append((0, [(name, 2, 1, 1, 0), (name, 0, 1, 1, 0)]))
    L = Loaded(dev, case)
    try:
        for flags in ALL_FLAGS:
            got = L.select(flags).read()
            want = L.model(flags)
            assert_selection(got, want, case["prefixes"], f"flags={flags}")
            for p in pinned:  # area 2 has rank 0
                if got[0][p] == rm.SEL_ROUTE:
                    assert case["prefixes"][p][1][got[2][p]][1] & rm.AREA_MASK == 2
            assert any(got[0][p] == rm.SEL_ROUTE for p in pinned)
            # the order matters: the identity order picks another advertisement somewhere
            ident = rm.select(case["prefixes"], case["areas"], case["me"], flags, np.arange(n_names),
                              np.arange(3), case["total_words"])
            assert np.any(ident[2] != want[2])
    finally:
        L.close()


# ---- prefix mirror ----------------------------------------------------------------

def _check_mirror(dev, ps, mirror, case, tab, flags, where):
    n = max(mirror) + 1 if mirror else 0
    prefixes = [mirror.get(p, (0, [])) for p in range(n)]
    n_pfx, live, pool = ps.info()
    assert n_pfx == n, where
    assert live == sum(len(a) for _, a in prefixes), where
    out = ra.Out(dev, n, case["total_words"])
    dev.ok(ps.select(case["me"], flags, tab, len(case["areas"]), out))
    want = rm.select(prefixes, case["areas"], case["me"], flags, case["name_rank"], case["area_rank"],
                     case["total_words"])
    assert_selection(out.read(), want, prefixes, where)
    out.free()
    return pool


def test_prefix_mirror_deltas(dev):
    """orh_prefix_load, then 20 rounds of orh_prefix_apply_delta (growth with
    gaps, withdrawals, lists that shrink and grow, one delta of 257 ids,
    enough churn to compact the pool): after every round the selection and
    orh_prefix_info equal a dict mirror's."""
    case = fuzz_case(3, 300, 3)
    rng = random.Random(77)
    flags = rm.SELECT_BEST_ROUTE | rm.SELECT_V4
    mirror = dict(enumerate(case["prefixes"]))
    ps = ra.PrefixSet(dev)
    tab = dev.areas(case["areas"])
    try:
        dev.ok(ps.load(case["prefixes"]))
        dev.ok(ps.set_order(case["name_rank"], case["area_rank"]))
        pools = [_check_mirror(dev, ps, mirror, case, tab, flags, "load")]
        compacted = False
        gaps_seen = False
        for rnd in range(20):
            n = max(mirror) + 1
            k = 257 if rnd == 7 else rng.randint(150, 250)
            ids = rng.sample(range(n), k - 6)
            top = n
            for _ in range(6):  # growth past the count, leaving gaps
                top += rng.randint(0, 3)
                ids.append(top)
                top += 1
            rng.shuffle(ids)
            new = []
            for p in ids:
                x = rng.random()
                old = mirror.get(p, (0, []))
                if x < 0.15:
                    e = (old[0], [])                     # withdrawn
                elif x < 0.3 and len(old[1]) > 1:
                    e = (old[0], old[1][:-1])            # shrinks
                else:
                    e = rand_prefix(rng, case["areas"], case["n_names"], case["me"])
                new.append(e)
                mirror[p] = e
            dev.ok(ps.delta(ids, new))
            gaps_seen |= any(p not in mirror for p in range(max(mirror) + 1))
            pools.append(_check_mirror(dev, ps, mirror, case, tab, flags, f"round {rnd}"))
            # a delta appends its records: a smaller pool was rebuilt from the live runs
            grown = pools[-2] + sum(len(a) for _, a in new)
            live = sum(len(a) for _, a in mirror.values())
            if pools[-1] < grown:
                assert grown > 4096 and grown > 2 * live and pools[-1] == live, (rnd, pools)
                compacted = True
        assert gaps_seen and compacted, pools
    finally:
        ps.close()


def test_prefix_delta_duplicate_ids(dev):
    """An id given three times in one delta: its last list wins on the host
    mirror and on the device, and the live count is exact."""
    case = fuzz_case(4, 300, 1)
    flags = rm.SELECT_BEST_ROUTE | rm.SELECT_V4
    A = case["areas"][0]
    good = [name for name in range(case["n_names"]) if name != case["me"] and A["name_node"][name] != rm.NO_NODE
            and A["dist"][A["name_node"][name]] != rm.UNREACHABLE and A["nh"][A["name_node"][name]].any()]
    a, b, c = good[:3]
    mirror = dict(enumerate(case["prefixes"]))
    ps = ra.PrefixSet(dev)
    tab = dev.areas(case["areas"])
    try:
        dev.ok(ps.load(case["prefixes"]))
        dev.ok(ps.set_order(case["name_rank"], case["area_rank"]))
        for rnd, target in enumerate((5, 299, 310)):  # an old id, the last one, a new one
            ids, new = [], []
            for p in range(10, 290):  # a delta of more than one block, the id at both ends and inside
                ids.append(p)
                new.append(mirror[p])
            lists = [(0, [(a, 0, 0, 0, 0)]), (0, [(b, 0, 0, 0, 0), (a, 0, 0, 0, 0), (c, 0, 0, 0, 0)]),
                     (0, [(c, 0, 1, 0, 0), (b, 0, 0, 0, 0)])]
            for at, e in zip((0, 130, len(ids) + 2), lists):
                ids.insert(at, target)
                new.insert(at, e)
            dev.ok(ps.delta(ids, new))
            mirror[target] = lists[-1]
            _check_mirror(dev, ps, mirror, case, tab, flags, f"duplicate round {rnd}")
            # the last list chose c alone
            out = ra.Out(dev, max(mirror) + 1, case["total_words"])
            dev.ok(ps.select(case["me"], flags, tab, 1, out))
            s, m, bst, k = out.read()
            assert (s[target], m[target], bst[target]) == (1, A["dist"][A["name_node"][c]], 0)
            assert np.array_equal(k[target], A["nh"][A["name_node"][c]])
    finally:
        ps.close()


# ---- route diff ---------------------------------------------------------------------

def _diff_check(dev, L, cur, prev, n, where):
    tw = cur.tw
    cur_h, prev_h = cur.read(), prev.read()
    for prev_n in (n, 1000, 0):
        d_changed = dev.alloc(4 * n * (4 + tw), ra.FILL)
        d_count = dev.alloc(4, ra.FILL)
        dev.ok(L.ps.diff(n, prev_n, cur, prev, d_changed, d_count))
        count = int(dev.get(d_count, np.uint32, 1)[0])
        raw = dev.get(d_changed, np.uint32, n * (4 + tw))
        recs = raw.reshape(n, 4 + tw)
        want = rm.diff(cur_h, prev_h, n, prev_n)
        got = {tuple(int(x) for x in r) for r in recs[:count]}
        assert count == len(want), (where, prev_n, count, len(want))
        assert len({r[0] for r in got}) == count, (where, prev_n, "an id twice")
        assert got == want, (where, prev_n)
        assert np.all(recs[count:].view(np.uint8) == ra.FILL), (where, prev_n, "wrote past the count")
        dev.free(d_changed, d_count)
    return len(rm.diff(cur_h, prev_h, n, n))


def test_route_diff(dev):
    n = 1025
    case = fuzz_case(5, n, 1)  # one area of three words
    assert case["total_words"] == 3
    flags = rm.SELECT_BEST_ROUTE | rm.SELECT_V4
    L = Loaded(dev, case)
    try:
        cur = L.select(flags)
        base = cur.read()
        assert_selection(base, L.model(flags), case["prefixes"])
        status = base[0]
        routes = np.nonzero(status == rm.SEL_ROUTE)[0]
        nones = np.nonzero(status == rm.SEL_NONE)[0]
        assert len(nones) > 4

        def variant(edit):
            s, m, b, k = (a.copy() for a in base)
            edit(s, m, b, k)
            out = ra.Out(dev, n, 3)
            out.write(s, m, b, k)
            return out

        def differ(s, m, b, k, p):  # any difference that is one: the status of a non-route, else the metric
            if s[p] == rm.SEL_ROUTE:
                m[p] += 1
            else:
                s[p] = rm.SEL_HOST if s[p] == rm.SEL_NONE else rm.SEL_NONE

        # nothing differs but stale words of NONE records: not reported, d_changed untouched
        def stale(s, m, b, k):
            for p in nones:
                m[p], b[p], k[p, 2] = 7, 3, 0xDEAD
        assert _diff_check(dev, L, cur, variant(stale), n, "stale") == 0

        # exactly one prefix per wave, at a varying lane
        def one_per_wave(s, m, b, k):
            stale(s, m, b, k)
            for w in range((n + 63) // 64):
                differ(s, m, b, k, min(w * 64 + (w * 37) % 64, n - 1))
        assert _diff_check(dev, L, cur, variant(one_per_wave), n, "one per wave") == 17

        # every prefix of wave 3; lanes 0 and 63 of wave 5; the last prefix alone in its wave
        def waves(s, m, b, k):
            for p in list(range(192, 256)) + [320, 383, 1024]:
                differ(s, m, b, k, p)
        assert _diff_check(dev, L, cur, variant(waves), n, "waves") == 67

        # single fields of a route: status, metric, best, the last mask word
        r = [int(p) for p in routes[:40:10]]

        def fields(s, m, b, k):
            s[r[0]] = rm.SEL_HOST
            m[r[1]] ^= 0x80000000
            b[r[2]] += 1
            k[r[3], 2] ^= 1
        assert _diff_check(dev, L, cur, variant(fields), n, "fields") == 4

        # and a selection after the rows changed
        A = case["areas"][0]
        rng = random.Random(9)
        for v in rng.sample(range(len(A["dist"])), 6):
            if v != A["name_node"][case["me"]]:
                A["dist"][v] = rng.randint(1, 12)
                A["nh"][v, 2] ^= 0x10
        L2 = Loaded(dev, case)
        prev = L2.select(flags)
        assert_selection(prev.read(), L2.model(flags), case["prefixes"])
        assert _diff_check(dev, L, cur, prev, n, "reselect") > 20
        L2.close()

        two = ra.Out(dev, n, 2)
        assert L.ps.diff(n, n, cur, two, dev.alloc(4 * n * 7), dev.alloc(4)) == ra.E_INVALID
    finally:
        L.close()


# ---- RibPolicy ------------------------------------------------------------------------

def make_policy(rng, n_stmts, n_prefix, total_words, tags=True, keep_nothing=False, more_ids=()):
    kinds = [("t", "p", "tp", "")[(s + s // 4) % 4] for s in range(n_stmts)]
    if not tags:
        kinds = [k.replace("t", "") for k in kinds]
    stmt_tags = sum(1 << s for s, k in enumerate(kinds) if "t" in k)
    stmt_pfx = sum(1 << s for s, k in enumerate(kinds) if "p" in k)
    ids = sorted(set(rng.sample(range(n_prefix), min(n_prefix, 120))) | {0, n_prefix - 1, n_prefix + 5} | set(more_ids))
    keep = [[0 if keep_nothing or rng.random() < 0.2 else rng.getrandbits(32) & rng.getrandbits(32)
             for _ in range(total_words)] for _ in range(n_stmts)]
    return dict(n_stmts=n_stmts, stmt_tags=stmt_tags, stmt_prefixes=stmt_pfx,
                tagset_stmts=[rng.getrandbits(32) & rng.getrandbits(32) for _ in range(N_TAGSETS)],
                pfx_id=ids, pfx_stmts=[rng.getrandbits(32) | rng.getrandbits(32) for _ in ids], keep=keep)


@pytest.fixture(scope="module")
def policy_case(dev):
    case = fuzz_case(6, 1025, 3)
    flags = rm.SELECT_BEST_ROUTE | rm.SELECT_V4
    L = Loaded(dev, case)
    sel = L.select(flags)
    sel_h = sel.read()
    assert_selection(sel_h, L.model(flags), case["prefixes"])
    yield L, sel, sel_h
    L.close()


def _policy_check(dev, L, sel, sel_h, pol, lo, hi, ranged=True):
    n, tw = L.n, L.case["total_words"]
    d_out, d_inv = dev.alloc(n, ra.FILL), dev.alloc(4, ra.FILL)
    dev.ok(L.ps.policy(lo, hi, sel, pol, tw, d_out, d_inv, ranged))
    got = dev.get(d_out, np.uint8, n)
    inv = int(dev.get(d_inv, np.uint32, 1)[0])
    dev.free(d_out, d_inv)
    want, want_inv = rm.policy(sel_h, [a for _, a in L.case["prefixes"]], pol, lo, hi)
    assert np.array_equal(got[lo:hi], want), np.nonzero(got[lo:hi] != want)[0][:8]
    assert np.all(got[:lo] == ra.FILL) and np.all(got[hi:] == ra.FILL)
    assert inv == want_inv
    return want, want_inv


@pytest.mark.parametrize("tags", [True, False])
@pytest.mark.parametrize("n_stmts", [0, 1, 31, 32])
def test_route_policy(dev, policy_case, n_stmts, tags):
    L, sel, sel_h = policy_case
    rng = random.Random(100 + n_stmts)
    pol = make_policy(rng, n_stmts, L.n, L.case["total_words"], tags=tags)
    want, inv = _policy_check(dev, L, sel, sel_h, pol, 0, L.n, ranged=False)
    routes = sel_h[0] == rm.SEL_ROUTE
    ovf = np.array([r and (a[int(b)][1] >> rm.TAGSET_SHIFT) == rm.TAGSET_OVF
                    for r, b, (_, a) in zip(routes, sel_h[2], L.case["prefixes"])])
    assert ovf.sum() > 10
    if n_stmts >= 31 and tags:
        assert inv > 0 and len(set(want.tolist())) > 8
        assert want.max() == rm.POL_NONE and rm.POL_HOST in want
        assert any(s >= 24 for s in want.tolist() if s < 32)
    if tags and n_stmts:
        assert np.all(want[ovf] == rm.POL_HOST)  # a tag statement and no id for the tags
    else:
        assert rm.POL_HOST not in want           # only prefix statements: decided here
    assert np.all(want[~routes] == rm.POL_NONE)


def test_route_policy_every_match_misses(dev, policy_case):
    """keep rows that miss every mask: each matching statement invalidates
    the route once and none applies."""
    L, sel, sel_h = policy_case
    pol = make_policy(random.Random(8), 32, L.n, L.case["total_words"], keep_nothing=True)
    want, inv = _policy_check(dev, L, sel, sel_h, pol, 0, L.n)
    assert set(want.tolist()) <= {rm.POL_NONE, rm.POL_HOST}
    assert inv > int((sel_h[0] == rm.SEL_ROUTE).sum())  # more than once for many routes


def test_route_policy_range_and_argument_errors(dev, policy_case):
    L, sel, sel_h = policy_case
    tw = L.case["total_words"]
    pol = make_policy(random.Random(9), 32, L.n, tw, more_ids=(255, 256))
    _, inv_all = _policy_check(dev, L, sel, sel_h, pol, 0, L.n)
    _, inv = _policy_check(dev, L, sel, sel_h, pol, 255, 257)
    assert inv <= inv_all
    _policy_check(dev, L, sel, sel_h, pol, 300, 300)
    d_out, d_inv = dev.alloc(L.n), dev.alloc(4)
    assert L.ps.policy(0, L.n, sel, dict(pol, n_stmts=33, keep=pol["keep"] + [[0] * tw]), tw, d_out,
                       d_inv) == ra.E_UNSUPPORTED
    unsorted = dict(pol, pfx_id=pol["pfx_id"][:5][::-1], pfx_stmts=pol["pfx_stmts"][:5])
    assert L.ps.policy(0, L.n, sel, unsorted, tw, d_out, d_inv) == ra.E_INVALID
    twice = dict(pol, pfx_id=[3, 3], pfx_stmts=[1, 1])
    assert L.ps.policy(0, L.n, sel, twice, tw, d_out, d_inv) == ra.E_INVALID
    assert L.ps.policy(0, L.n + 1, sel, pol, tw, d_out, d_inv) == ra.E_INVALID
    assert L.ps.policy(0, L.n, sel, pol, tw + 1, d_out, d_inv) == ra.E_INVALID
