"""Graphs at the word and bucket edges of the HBM frontier searches
(spf_global_kernel, spf_global_nh_async_kernel) and the plain models that
say what each graph makes those kernels do. No GPU; imported by
test_hbm_shapes.py (which pins the properties on the CPU oracle), by
test_gpu_hbm_edges.py and by its child processes.

Both kernels keep a node per bit in near / far bitmaps of NB = ceil(N / 32)
words and advance a threshold T in steps of delta = mean live metric *
ORH_DELTA_PCT / 100 (at least 1; the metric itself when uniform):

  two_scale_ring   N = 613 (NB = 20, 5 nodes in the last word): metrics of 1
                   and of 50,000+, so delta is tiny against the chords (they
                   are pushed far and lowered later round the ring) or huge
                   against the ring, by ORH_DELTA_PCT
  ecmp_grid        23 x 23, metrics 1..3 in a pattern with many equal-cost
                   paths: equal-distance mask merges
  hubs             a hub of exactly 32 distinct neighbours (first-hop bit 31,
                   parallel links, overflow records) and one of 40 (two words)
  wan              8,229 nodes (NB = 258 > 256 threads) and 32,805 (NB = 1,026
                   > 1,024 threads): a thread owns a second bitmap word
  tiny             20 nodes: NB = 1, a one-word ignore filter
"""
import random

from openr_amd.topology import int_topology, wan

RING_N, RING_CYCLE = 613, 600
RING_CHORDS = [37 * k for k in range(1, 17)]
RING_CHORD_METRIC, RING_SPUR_METRIC = 50_000, 60_000
GRID = 23
GRID_OVERLOADED, GRID_DRAINED, GRID_ISOLATED = 11 * GRID + 11, (5 * GRID + 5, 5 * GRID + 6), GRID * GRID
HUB_N, HUB_A, HUB_B = 200, 0, 100
WAN_SMALL, WAN_LARGE, WAN_SEED = 8229, 32805, 11


def _link(adj, a, b, w_ab, w_ba=None):
    adj[a].append((b, w_ab))
    adj[b].append((a, w_ab if w_ba is None else w_ba))


def two_scale_ring():
    """Ring 0..599 at metric 1, chords 0 - 37k (k = 1..16) at 50,000, the link
    300 - 600 at 60,000 and the chain 600..612 at metric 7. 1,258 up CSR
    entries whose metrics sum to 1,721,368: the mean is 1,368."""
    adj = {i: [] for i in range(RING_N)}
    for i in range(RING_CYCLE):
        _link(adj, i, (i + 1) % RING_CYCLE, 1)
    for c in RING_CHORDS:
        _link(adj, 0, c, RING_CHORD_METRIC)
    _link(adj, 300, RING_CYCLE, RING_SPUR_METRIC)
    for i in range(RING_CYCLE, RING_N - 1):
        _link(adj, i, i + 1, 7)
    return int_topology(adj)


def ring_few_sources():
    """40 seeded ring nodes and 0 (the chords' hub), 300 (the spur), 612 (the
    chain's end, in the partial last word): 43 sources."""
    fixed = ["0", "300", "612"]
    rest = [str(i) for i in range(RING_N) if str(i) not in fixed]
    return random.Random(3000).sample(rest, 40) + fixed


# a chord end, a node next to the spur, the spur, the ring's last node, the chain's end
RING_TWO_PHASE_SOURCES = ["0", "37", "296", "300", "599", "612"]


def ecmp_grid(defects=False):
    """23 x 23, node r * 23 + c. (r, c) - (r, c + 1) costs 1 + (r + c) % 3 and
    (r, c) - (r + 1, c) costs 1 + (r + 2c) % 3, the same both ways. With
    ``defects``: node (11, 11) overloaded, the link (5, 5) - (5, 6) drained
    from its left end, and an extra node 529 with no link at all."""
    n = GRID
    adj = {i: [] for i in range(n * n + (1 if defects else 0))}
    for r in range(n):
        for c in range(n):
            if c + 1 < n:
                _link(adj, r * n + c, r * n + c + 1, 1 + (r + c) % 3)
            if r + 1 < n:
                _link(adj, r * n + c, (r + 1) * n + c, 1 + (r + 2 * c) % 3)
    dbs = int_topology(adj)
    if defects:
        for db in dbs:
            if db.thisNodeName == str(GRID_OVERLOADED):
                db.isOverloaded = True
            if db.thisNodeName == str(GRID_DRAINED[0]):
                for a in db.adjacencies:
                    if a.otherNodeName == str(GRID_DRAINED[1]):
                        a.isOverloaded = True
    return dbs


def hubs():
    """A ring of 200 nodes with seeded metrics 1..9 per direction. Hub A = 0
    has its two ring neighbours and 30 spokes (32 distinct neighbours) and a
    second, parallel link to two of the spoke ends: 34 records, so its ELL row
    ends in a continuation record at either width. Hub B = 100 has 40
    distinct neighbours (two mask words)."""
    rng = random.Random(3100)
    n = HUB_N
    adj = {i: [] for i in range(n)}
    for i in range(n):
        _link(adj, i, (i + 1) % n, rng.randint(1, 9), rng.randint(1, 9))
    spokes_a = [5 + 6 * k for k in range(30)]           # 5, 11, .., 179
    spokes_b = [(HUB_B + 3 + 4 * k) % n for k in range(38)]  # 103, 107, .., 51
    assert not set(spokes_a) & {1, n - 1, HUB_B} and not set(spokes_b) & {HUB_B - 1, HUB_B + 1, HUB_A}
    for v in spokes_a:
        _link(adj, HUB_A, v, 1, rng.randint(1, 9))
    for v in (spokes_a[3], spokes_a[-1]):
        _link(adj, HUB_A, v, rng.randint(2, 9), rng.randint(1, 9))
    for v in spokes_b:
        _link(adj, HUB_B, v, 1, rng.randint(1, 9))
    # a hub's own side of every first link to a neighbour costs 1, so from the
    # hub each neighbour's first-hop set holds its own rank, whatever order
    # the ranks are given in: bit 31 of A's word and B's second word are used
    for hub in (HUB_A, HUB_B):
        for k in (0, 1):
            nb, _ = adj[hub][k]
            adj[hub][k] = (nb, 1)
    return int_topology(adj)


def hub_neighbours(dbs, node):
    """Distinct neighbours of ``node`` (an int) in ``dbs``."""
    db = next(d for d in dbs if d.thisNodeName == str(node))
    return {a.otherNodeName for a in db.adjacencies}


def wan_small():
    return wan(WAN_SMALL, seed=WAN_SEED)[0]


def wan_large():
    return wan(WAN_LARGE, seed=WAN_SEED)[0]


def tiny():
    """20 nodes: a seeded spanning tree plus 12 seeded extra links, metrics
    1..9 per direction."""
    rng = random.Random(3200)
    n = 20
    adj = {i: [] for i in range(n)}
    links = set()
    for i in range(1, n):
        links.add((rng.randrange(i), i))
    while len(links) < n - 1 + 12:
        a, b = rng.randrange(n), rng.randrange(n)
        if a != b and (a, b) not in links and (b, a) not in links:
            links.add((a, b))
    for a, b in sorted(links):
        _link(adj, a, b, rng.randint(1, 9), rng.randint(1, 9))
    return int_topology(adj)


def drain_grid():
    """test_drain_tiers' 60 x 60 layout (node r * 60 + c) with horizontal
    links at metric 1 and vertical ones at 2: general metrics whose mean
    live metric is 1, so the what-if job's full search runs at delta = 1."""
    n = 60
    adj = {i: [] for i in range(n * n)}
    for r in range(n):
        for c in range(n):
            if c + 1 < n:
                _link(adj, r * n + c, r * n + c + 1, 1)
            if r + 1 < n:
                _link(adj, r * n + c, (r + 1) * n + c, 2)
    return int_topology(adj)


def mean_live_metric(dbs):
    """The integer mean of w_out over the up CSR entries, as orh_graph_load
    computes mean_out: an adjacency is an entry once its other end reports
    the same link back, and it is up unless either end drained it."""
    ends = {}
    for db in dbs:
        for a in db.adjacencies:
            ends[(db.thisNodeName, a.ifName, a.otherNodeName, a.otherIfName)] = a
    total = count = 0
    for (node, ifn, other, oif), a in ends.items():
        back = ends.get((other, oif, node, ifn))
        if back is None or a.isOverloaded or back.isOverloaded:
            continue
        total += a.metric
        count += 1
    return total // count if count else 1


def delta_of(dbs, pct=50):
    """The kernels' bucket width on a graph of general metrics at
    ORH_DELTA_PCT = pct (50 is the product's default)."""
    return max(1, mean_live_metric(dbs) * pct // 100)


def bucket_walk(dist_row, delta):
    """(advances, jumps) of a delta-stepping search whose final distances are
    ``dist_row`` (unreached entries 0xFFFFFFFF are left out): the threshold
    starts at delta; while some distance is >= T the smallest such, m, is the
    next far minimum, T becomes m + delta (an advance), and the step is a jump
    when m lies more than delta past T, i.e. whole bucket widths were empty."""
    ds = sorted(int(d) for d in dist_row if int(d) != 0xFFFFFFFF)
    delta = int(delta)
    T, advances, jumps, k = delta, 0, 0, 0
    while True:
        while k < len(ds) and ds[k] < T:
            k += 1
        if k == len(ds):
            return advances, jumps
        m = ds[k]
        advances += 1
        if m - T > delta:
            jumps += 1
        T = m + delta
