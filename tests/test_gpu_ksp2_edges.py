"""The KSP2 device traces (ksp_kernels.hip) at their capacity bounds, on both
trace kernels, over high-degree nodes and both ELL widths, and through the
batching switches (``-m gpu``). Every pair's k = 1 and k = 2 paths equal the
oracle's getKthPaths (LinkState.cpp:762-791) on the same adjacency databases
loaded in the same order, link by link and in order; ksp_stats() equals the
(device, host) split derived from the caps in the code.

The caps (api/ksp.hip orh_ksp2_batch, ksp_kernels.hip):

  per pair        wave kernel (default)    thread kernel (ORH_KSP_WAVE=0)
  DFS frames      kWaveStack = 512         kKspStackCap = 1024
  visited slots   kWaveHash  = 1024        kKspHashCap  = 2048
  ignore links    kKspIgnCap = 512         kKspIgnCap   = 512
  block words     kKspOutCap = 1024        kKspOutCap   = 1024

and the checks that flag a pair (status word 1: the host traces it, k = 1 and
k = 2 both), the same in both kernels:

  frames   a link consumed at depth `top` (frames 0..top hold the way from the
           destination) is flagged when top + 1 >= stack cap: a path of L links
           consumes its last link at top = L - 1, so L <= cap - 1 stays.
  visited  visit() refuses - before it looks the link up - once
           2 * (count + 1) > slots: the set takes slots / 2 links, and any
           visit after that, of a link already in it too, flags the pair. So
           slots / 2 - 1 links always stay, and slots / 2 stay only when no
           visit follows the last insertion.
  ignore   a found k = 1 path is flagged when the k = 1 links so far plus its
           own exceed 512.
  block    a found path of len links is flagged when w + 1 + len + 1 > 1024,
           w the next free word: the block starts [status, offset of the k = 2
           section], a section is [paths, then len and the links of each].

The wave kernel does not use the stack_cap / hash_cap it is passed (1024 /
2048): its stack and visited set are LDS arrays of kWaveStack / kWaveHash, so
the two kernels flag different pairs; tests/ksp2_shapes.py holds both sets.
"""
import json
import os
import subprocess
import sys

import pytest

import ksp2_shapes as shapes
from openr_amd.facade import LinkDesc, load_topology
from openr_amd.types import K_TESTING_AREA

from test_gpu_parity import random_topology

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SWITCHES = ("ORH_KSP_WAVE", "ORH_KSP_ORDER", "ORH_KSP_CHUNK", "ORH_KSP_STOP", "ORH_KSP_HOST", "ORH_KSP_LDS",
             "ORH_KSP_PROF")


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)


_SHAPES, _WANT = {}, {}


def _shape(name):
    if name not in _SHAPES:
        _SHAPES[name] = shapes.SHAPES[name]()
        assert len(set(_SHAPES[name]["pairs"])) == len(_SHAPES[name]["pairs"])
    return _SHAPES[name]


def _want(oracle, name):
    """The oracle's paths of the shape's pairs and its spf_runs over them
    (one per source, one per pair with k = 1 paths), computed once."""
    if name not in _WANT:
        sh = _shape(name)
        als_o, _ = load_topology(oracle, sh["dbs"], [])
        runs0 = als_o[A]._impl.spf_runs
        paths = {(s, d, k): als_o[A].get_kth_paths(s, d, k) for s, d in sh["pairs"] for k in (1, 2)}
        _WANT[name] = (paths, als_o[A]._impl.spf_runs - runs0)
    return _WANT[name]


def _check_shape(hip, oracle, name, host_key="host_wave"):
    sh = _shape(name)
    want, want_runs = _want(oracle, name)
    als_h, _ = load_topology(hip, sh["dbs"], [])
    ls = als_h[A]._impl
    runs0 = ls.spf_runs
    ls.prefetch_kth_paths(sh["pairs"])
    stats = ls.ksp_stats()
    print(name, "ksp_stats", stats, "expected host", sorted(sh[host_key]))
    for s, d in sh["pairs"]:
        for k in (1, 2):
            assert als_h[A].get_kth_paths(s, d, k) == want[(s, d, k)], (name, s, d, k)
    assert sh[host_key] <= set(sh["pairs"])
    assert stats == (len(sh["pairs"]) - len(sh[host_key]), len(sh[host_key])), name
    assert ls.spf_runs - runs0 == want_runs, name
    return want


# ---- 1. capacity bounds, wave kernel ------------------------------------------

def test_path_graph_stack_bound(hip, oracle):
    """A path graph of 520 nodes, metric 1: one k = 1 path of L links, no
    k = 2. Wave kernel: frames, L <= 511 (top + 1 >= 512 at the last link of
    L = 512), and the visited set says the same: 512 links fill it and the
    first visit of the next trace is refused, so the frame test never decides
    alone (a frame is pushed per inserted link, and kWaveStack is half of
    kWaveHash; likewise 1,024 of 2,048 in the thread kernel). The ignore list
    and the block are further out (511 links, 3 + 1 + L words). So (p0, p511) and its reverse stay on the
    device, (p0, p512), (p0, p513) and their reverses go to the host (thread
    kernel: 1,024 frames, so the ignore list decides, L <= 512). p0 has pairs
    on both sides: spf_runs counts its run once."""
    want = _check_shape(hip, oracle, "path")
    for s, d in _shape("path")["pairs"]:
        assert len(want[(s, d, 1)]) == 1 and want[(s, d, 2)] == []
    assert [len(want[("p0", f"p{n}", 1)][0]) for n in (511, 512, 513)] == [511, 512, 513]


def test_ring_k2_overflow(hip, oracle):
    """A ring of 612 nodes, metric 1: a pair d links apart has one k = 1 path
    of d links and one k = 2 path of 612 - d (d = 306: two k = 1 paths, no
    k = 2). Wave kernel frames, L <= 511: (r0, r101) stays with k = 2 at 511
    links; (r0, r100) is flagged by its k = 2 trace (512 links) after its
    k = 1 section was written, and the host redoes both; (r0, r1) likewise
    (611). (r0, r306) is flagged in k = 1 by both kernels: the second path
    makes 612 links, over the visited set's 512 (wave) and the ignore list's
    512 (thread). The other pairs are 101..305 apart and stay on the device.
    r0 has pairs on both sides: spf_runs counts its run once."""
    want = _check_shape(hip, oracle, "ring")
    assert [len(p) for p in want[("r0", "r306", 1)]] == [306, 306] and want[("r0", "r306", 2)] == []
    assert [len(want[("r0", "r100", k)][0]) for k in (1, 2)] == [100, 512]
    assert [len(want[("r0", "r101", k)][0]) for k in (1, 2)] == [101, 511]


def test_two_rings_ignore_bound(hip, oracle):
    """Rings of 512 and 514 nodes: the antipodal pair has two k = 1 paths of
    256 / 257 links. 512 links fill the ignore list exactly and stay in the
    thread kernel; the wave kernel's visited set holds them too, but the trace
    after the second path visits a consumed link with count = 512 and is
    refused, so it flags the pair. 514 links are flagged by both. (v1, v0) has
    k = 2 of 513 links: over the wave kernel's frames only; (u300, u301) has
    511 and stays."""
    want = _check_shape(hip, oracle, "two_rings")
    assert [len(p) for p in want[("u0", "u256", 1)]] == [256, 256]
    assert [len(p) for p in want[("v0", "v257", 1)]] == [257, 257]
    assert [len(p) for p in want[("u300", "u301", 2)]] == [511] and [len(p) for p in want[("v1", "v0", 2)]] == [513]


@pytest.mark.parametrize("length", [507, 508])
def test_theta_k2_block_bound(hip, oracle, length):
    """S - T by one link (k = 1: words 2..4, the k = 2 section from word 5)
    and by two ways of L links each (k = 2: the first path found at w = 6, the
    second at w = 7 + L, kept while 2 L + 9 <= 1024). The thread kernel keeps
    L = 507 and flags L = 508 (1,016 visited links fit its 2,048 slots); the
    wave kernel flags both through its visited set (over 512 links). The
    short pairs' k = 2 paths go round through S - T, up to 508 links, and
    stay on the device."""
    want = _check_shape(hip, oracle, f"theta{length}")
    assert [len(p) for p in want[("s", "t", 1)]] == [1] and [len(p) for p in want[("s", "t", 2)]] == [length] * 2
    assert [len(p) for p in want[("a1", "s", 2)]] == [length]


def test_fans_visited_and_ignore_bounds(hip, oracle):
    """Fans of M = 255, 256, 257 two-link paths S - m_i - T (S and T of degree
    M + 1: four or five candidate passes of 64 per step), and a three-link
    detour for k = 2. k = 1 of (S, T) consumes 2 M links and, after the last
    path, tries one more trace whose first visit (of a consumed link) comes
    with count = 2 M. Wave kernel, visited: 2 * (2 M + 1) <= 1024 holds for
    M = 255 only, so M = 256 is flagged although its 512 links fit the set -
    the refusal comes before the lookup - and M = 257 too. Thread kernel: 2,048
    slots, so the ignore list decides: 2 M <= 512 keeps M = 256 and flags 257.
    Failed branches count too: k = 2 of (x, T) consumes 3 links for its path
    and 2 for every other mid before it gives up, 511 for M = 255 (stays) and
    513 for M = 256 (flagged by the wave kernel, not by the thread kernel);
    k = 2 of (m_i, S) consumes 3 and 2 for each of the other M - 2 mids: 511
    for (f256m5, f256s), which stays, 513 for (f257m9, f257s), flagged by the
    wave kernel. Blocks: 3 + 3 M words."""
    want = _check_shape(hip, oracle, "fans")
    for m in shapes.FAN_SIZES:
        for s, d in ((f"f{m}s", f"f{m}t"), (f"f{m}t", f"f{m}s")):
            assert [len(p) for p in want[(s, d, 1)]] == [2] * m and [len(p) for p in want[(s, d, 2)]] == [3]


def test_big_fans_thread_visited_bound(hip, oracle):
    """Fans of M = 511 and 512 mids: k = 2 of (x, T) and of (y, S) finds one
    path of three links and consumes two more at every other mid before it
    gives up, 2 M + 1 in all, each insertion followed by another visit. The
    thread kernel's table takes 1,024: 1,023 stay (M = 511), 1,025 are flagged
    (M = 512; test_thread_per_pair_kernel). The wave kernel flags all four;
    the pairs next to them consume four links and stay."""
    want = _check_shape(hip, oracle, "big_fans")
    for m in (511, 512):
        assert [len(p) for p in want[(f"g{m}x", f"g{m}t", 2)]] == [3] == [len(p) for p in want[(f"g{m}y", f"g{m}s", 2)]]


def test_parallel_links_block_bound(hip, oracle):
    """M parallel links S - T of metric 1: k = 1 is M one-link paths, 2 words
    each from word 3, path j found with w = 3 + 2 j and kept while
    w + 3 <= 1024: j <= 509. Without a detour M = 510 stays (k = 1 ends at
    w = 1023, and the empty k = 2 section is the block's last word) and
    M = 511 is flagged in k = 1. With the two-link detour k = 2 has one path
    at w = 3 + 2 M + 1, kept while w + 4 <= 1024: M = 508 stays and M = 509 is
    flagged in k = 2. Both kernels (510 visited / ignore links fit either).
    (u, T) from the pendant u on S has one path, and its second trace consumes
    every parallel link on failing branches: M + 1 links, the visit after the
    last being refused by the wave kernel at M = 511 only (count = 512).
    Each bound pair is followed by a short pair of the same batch."""
    want = _check_shape(hip, oracle, "parallel")
    for name, m, detour in shapes.BUNDLES:
        for s, d in ((f"{name}s", f"{name}t"), (f"{name}t", f"{name}s")):
            assert [len(p) for p in want[(s, d, 1)]] == [1] * m
            assert [len(p) for p in want[(s, d, 2)]] == ([2] if detour else [])


# ---- 2. high-degree nodes, both ELL widths -------------------------------------

@pytest.mark.parametrize("ell", [4, 8])
def test_parallel_bundles_of_70(hip, oracle, ell):
    """S = 70 links = P = 70 links = T with directional metrics that tie: the
    70 candidates of a step share (dist, name rank) and differ in the record
    index only, over two passes of 64; 70 k = 1 paths pairing the bundles'
    links in LinkSet order. Pendant leaves keep the ninth-decile degree at 1
    (ell_k = 4: 3 inline records and 137 continuation records at P); a clique
    of 12 raises it to 11 (ell_k = 8)."""
    name = f"bundles70_ell{ell}"
    assert shapes.ell_width(_shape(name)["dbs"]) == ell
    want = _check_shape(hip, oracle, name)
    for s, d, n in (("S", "T", 2), ("T", "S", 2), ("S", "P", 1), ("P", "T", 1)):
        paths = want[(s, d, 1)]
        assert [len(p) for p in paths] == [n] * 70 and len({l for p in paths for l in p}) == 70 * n


@pytest.mark.parametrize("ell", [4, 8])
def test_hub_of_80(hip, oracle, ell):
    """A hub of degree 81 (two candidate passes at it) with chords that tie
    with or beat the way through it, parallel chords included; the pairs cross
    the hub, start at it and end at it."""
    name = f"hub80_ell{ell}"
    assert shapes.ell_width(_shape(name)["dbs"]) == ell
    want = _check_shape(hip, oracle, name)
    assert sum(len(v) for v in want.values()) > len(_shape(name)["pairs"])


def test_unreachable_and_drained(hip, oracle):
    """src == dst, a destination in another component, behind an overloaded
    node on the only ways there (no paths, and traced on the device, not
    flagged); an overloaded source and an overloaded destination (paths)."""
    sh = _shape("defects")
    assert shapes.ell_width(sh["dbs"]) == 4
    want = _check_shape(hip, oracle, "defects")
    for s, d in sh["pairs"]:
        assert (want[(s, d, 1)] == []) == ((s, d) in sh["empty"]), (s, d)
    assert want[("b", "e", 1)] and want[("a", "b", 1)] and want[("h", "a", 1)]


# ---- 3. batching and the switches read per call --------------------------------

def _all_pairs(hip, oracle, dbs, before=None):
    als_h, _ = load_topology(hip, dbs, [])
    als_o, _ = load_topology(oracle, dbs, [])
    names = sorted(db.thisNodeName for db in dbs)
    pairs = [(s, d) for s in names for d in names]
    ls = als_h[A]._impl
    runs0, runs_o0 = ls.spf_runs, als_o[A]._impl.spf_runs
    for s, d in before or []:
        assert als_h[A].get_kth_paths(s, d, 1) == als_o[A].get_kth_paths(s, d, 1), (s, d)
    ls.prefetch_kth_paths(pairs)
    stats = ls.ksp_stats()
    for s, d in pairs:
        for k in (1, 2):
            assert als_h[A].get_kth_paths(s, d, k) == als_o[A].get_kth_paths(s, d, k), (s, d, k)
    assert ls.spf_runs - runs0 == als_o[A]._impl.spf_runs - runs_o0
    return pairs, stats


def test_two_chunks_order_kernel_strided(hip, oracle):
    """All 2,116 pairs of a 46-node graph in one prefetchKthPaths: chunks of
    2,048 and 68 pairs, ksp_order_kernel at P = 2,048 (two rounds of its
    1,024-thread loops)."""
    dbs = random_topology(2400, n=46, extra=70, max_metric=4, parallel=0.4, overload=0.1, link_overload=0.06)
    pairs, stats = _all_pairs(hip, oracle, dbs)
    assert len(pairs) == 2116 and stats == (2116, 0)


@pytest.mark.parametrize("stop", [None, "0"])
def test_chunks_of_seven(hip, oracle, monkeypatch, stop):
    """ORH_KSP_CHUNK=7 over 400 pairs: 57 chunks of 7 and a last one of a
    single pair; again with ORH_KSP_STOP=0 (searches run to the end)."""
    monkeypatch.setenv("ORH_KSP_CHUNK", "7")
    if stop is not None:
        monkeypatch.setenv("ORH_KSP_STOP", stop)
    dbs = _shape("random")["dbs"]
    pairs, stats = _all_pairs(hip, oracle, dbs)
    assert len(pairs) == 400 and len(pairs) % 7 == 1 and stats == (400, 0)


def test_half_memoized_pairs(hip, oracle):
    """Every seventh pair of the first ten sources has its k = 1 paths
    memoized before the batch: those take the host path (k = 2 over a fresh
    SPF), the rest the device, and spf_runs still counts each source once,
    whether getKthPaths or the batch met it first."""
    dbs = _shape("random")["dbs"]
    names = sorted(db.thisNodeName for db in dbs)
    before = [(s, d) for s in names for d in names][3:200:7]
    pairs, stats = _all_pairs(hip, oracle, dbs, before)
    assert stats == (len(pairs) - len(before), len(before))


# ---- 4. the switches read once per process -------------------------------------

_CHILD = r"""
import json, sys, time
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import ksp2_shapes as shapes
from openr_amd import host_backend
from openr_amd.facade import load_topology
from openr_amd.types import K_TESTING_AREA as A
hip, out = host_backend(), {}
for name in sys.argv[4:]:
    sh = shapes.SHAPES[name]()
    als, _ = load_topology(hip, sh["dbs"], [])
    ls = als[A]._impl
    t0 = time.time()
    ls.prefetch_kth_paths(sh["pairs"])
    out[name] = dict(secs=time.time() - t0, stats=list(ls.ksp_stats()),
                     paths=[[ls.get_kth_paths(s, d, k) for k in (1, 2)] for s, d in sh["pairs"]])
with open(sys.argv[3], "w") as f:
    json.dump(out, f)
"""


def _child(tmp_path, oracle, switch, host_key, names):
    out = tmp_path / "paths.json"
    env = {k: v for k, v in os.environ.items() if k not in _SWITCHES}
    env[switch] = "0"
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, os.path.join(ROOT, "tests"), str(out)] + names,
                   check=True, env=env, timeout=120)
    with open(out) as f:
        got = json.load(f)
    for name in names:
        sh = _shape(name)
        want, _ = _want(oracle, name)
        print(name, "prefetch %.3f s" % got[name]["secs"], "ksp_stats", got[name]["stats"])
        for (s, d), ks in zip(sh["pairs"], got[name]["paths"]):
            for k in (1, 2):
                assert [[LinkDesc(*l) for l in p] for p in ks[k - 1]] == want[(s, d, k)], (name, s, d, k)
        n = len(sh["pairs"])
        assert got[name]["stats"] == [n - len(sh[host_key]), len(sh[host_key])], name


def test_thread_per_pair_kernel(oracle, tmp_path):
    """ORH_KSP_WAVE=0 (read once per process, hence the child):
    ksp_trace_kernel<4|8> with its own visited table (2,048 slots), stack in
    global memory (1,024 frames) and insertion sort of the ignore set, over
    the shapes above and a 20-node all-pairs batch. Its bounds: the ignore
    list before the frames on the path graph (L = 512 stays, 513 is flagged),
    on the two rings (2 x 256 stay, 2 x 257 are flagged) and on the fans
    (M = 256 stays, 257 is flagged); the rings' k = 2 paths of 512, 513 and
    611 links stay; its visited table on the big fans (1,023 links stay,
    1,025 are flagged); the block bound on the theta graphs (k = 2 of 2 x 507
    links stays, 2 x 508 is flagged). The 508..511 parallel links are left to
    the wave kernel: a lane re-scans all of a node's records at every step
    and a trace steps over every consumed link again, which took this kernel
    39 s there (the fans take it 6 s of this test's 9; the wave kernel 1.3 s
    and 0.3 s)."""
    names = [n for n in shapes.SHAPES if n != "parallel"]
    _child(tmp_path, oracle, "ORH_KSP_WAVE", "host_thread", names)


def test_pair_order_searches(oracle, tmp_path):
    """ORH_KSP_ORDER=0 (read once per process): the k = 2 searches in pair
    order, without ksp_order_kernel; the same paths and the wave kernel's
    split on every shape."""
    _child(tmp_path, oracle, "ORH_KSP_ORDER", "host_wave", list(shapes.SHAPES))
