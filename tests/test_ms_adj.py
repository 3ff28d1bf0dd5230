"""The slice adjacency of the multi-source BFS layout (ms_slice_adjacency,
csrc/host/ms_order.h) without a device: the C++ function through
`_openr_host.ms_slice_adjacency` against its restatement in
tools/ms_order_model.py, in the cluster order the library builds; every slice
holds itself; the kernel's bitmask words say the same; and the model's replay
of the all-sources sweep with the library's adjacency meets no arrival
outside the slices the adjacency skip would run (replay asserts it on every
level)."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORDS = 8  # kMsAdjWords: 256 slices


def _load_model():
    spec = importlib.util.spec_from_file_location("ms_order_model", os.path.join(ROOT, "tools", "ms_order_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


model = _load_model()

GRAPHS = {
    "grid40": lambda: model.grid(40),
    "ring2011_k4": lambda: model.ring_with_chords(2011, 4),
}


@pytest.fixture(scope="module")
def host():
    from openr_amd import _openr_host
    return _openr_host


@pytest.fixture(scope="module", params=sorted(GRAPHS))
def case(request, host):
    adj = GRAPHS[request.param]()
    _, _, cluster = host.ms_orders(adj)
    lists, words = host.ms_slice_adjacency(adj, cluster)
    return adj, list(cluster), [list(x) for x in lists], list(words)


def test_adjacency_matches_the_model(case):
    adj, order, lists, _ = case
    assert len(lists) == (len(adj) + 63) // 64
    assert lists == model.slice_adjacency(adj, order)


def test_every_slice_holds_itself_and_lists_ascend(case):
    _, _, lists, _ = case
    for s, lst in enumerate(lists):
        assert s in lst
        assert lst == sorted(set(lst)) and lst[-1] < len(lists)


def test_adjacency_is_symmetric(case):
    """Links are two-way, so slice a is adjacent to b iff b is to a."""
    _, _, lists, _ = case
    for s, lst in enumerate(lists):
        assert all(s in lists[t] for t in lst)


def test_mask_words_say_the_same(case):
    _, _, lists, words = case
    assert len(words) == WORDS * len(lists)
    for s, lst in enumerate(lists):
        row = words[WORDS * s:WORDS * (s + 1)]
        assert [t for t in range(32 * WORDS) if (row[t // 32] >> (t % 32)) & 1] == lst


def test_replay_meets_no_arrival_outside_the_needed_slices(case):
    adj, order, lists, _ = case
    r = model.replay(adj, order, lists)
    print({k: r[k] for k in ("open", "need", "arrive", "open_g", "need_g", "crit_open", "crit_need")})
    assert r["arrive"] <= r["need"] <= r["open"]
    assert r["need_g"] <= r["open_g"] and r["crit_need"] <= r["crit_open"]


def test_repeats_down_links_and_self_entries_are_taken(host):
    """The layout hands over every CSR record: repeats (parallel links), a
    free slot's own id, and - being records like any other - down links."""
    n = 130  # three slices in the identity order
    adj = [[] for _ in range(n)]
    adj[0] = [0, 129, 129]
    adj[129] = [0]
    adj[70] = [70]
    lists, words = host.ms_slice_adjacency(adj, list(range(n)))
    assert [list(x) for x in lists] == [[0, 2], [1], [0, 2]]
    assert len(words) == 3 * WORDS and words[0] == 0b101 and words[WORDS] == 0b010


def test_past_the_envelope_there_are_no_words(host):
    for n, slices in ((64 * 32 * WORDS, 256), (64 * 32 * WORDS + 1, 257)):
        adj = [[(v + 1) % n, (v - 1) % n] for v in range(n)]
        lists, words = host.ms_slice_adjacency(adj, list(range(n)))
        assert len(lists) == slices and len(words) == (slices * WORDS if slices <= 256 else 0)


def test_bad_orders_are_refused(host):
    with pytest.raises(ValueError):
        host.ms_slice_adjacency([[1], [0]], [0, 0])
    with pytest.raises(ValueError):
        host.ms_slice_adjacency([[1], [0]], [0])
    with pytest.raises(ValueError):
        host.ms_slice_adjacency([[2], [0]], [0, 1])
