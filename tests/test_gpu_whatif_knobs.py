"""The what-if paths that only an environment switch reaches (``-m gpu``):
ORH_WHATIF_T3_SPLIT=0 (the slot tier on the side stream), ORH_WHATIF_FULL=n
(full searches for the head of the slot tier's queue, tier 2 skipped in front
of them), ORH_WHATIF_SKIP_T2=0 (tier 2 kept), and a run with metric raises
under ORH_WHATIF_FULL, which takes no full search. ORH_REPAIR_CAPS (the tiers'
caps, the two-tier plan, full searches behind it) has test_gpu_whatif_caps.py.

The switches are read once per process, so every setting runs in a child
process of its own. The job is test_drain_tiers' (test_gpu_whatif_drain.py):
a 60x60 grid, sources 0 and 1830, 114 drain requests that show tiers 0 to 3
and overflow the 64 slots. A child writes helpers.row_digest of every
request's row and its info word (tier | affected << 3); the parent compares
the digests with the oracle's rows, one request of each distinct kind, the
repeated requests with each other.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from openr_amd.facade import load_topology
from openr_amd.topology import bench_grid
from openr_amd.types import K_TESTING_AREA

from helpers import row_digest
from test_gpu_whatif_drain import Oracles
from test_gpu_whatif_impact import to_row
from test_gpu_whatif_metric import Oracles as RaiseOracles

pytestmark = pytest.mark.gpu
A = K_TESTING_AREA
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = ["0", "1830"]
FAR = [str(r * 60 + c) for r in range(54, 60) for c in range(53, 60)]
# test_drain_tiers' requests: (source index, drained node)
DRAINS = [(0, "1")] * 35 + [(1, "1831")] + [(0, x) for x in FAR] + [(0, "1")] * 35
BIG = [i for i, r in enumerate(DRAINS) if r == (0, "1")]
MID = 35  # (1, "1831"): the lone tier-2 request
# what test_drain_tiers asserts of the default run, as info words
DEFAULT_INFO = np.array([3 | 3539 << 3 if r == (0, "1") else 2 | 1739 << 3 if r == (1, "1831") else 0
                         for r in DRAINS], dtype=np.uint32)
# the raises: (source index, tail, head, metric); 0 -> 1 and 1830 -> 1831 are
# test_raise_tiers' tier-3 and tier-2 cases (3,540 and 1,740 nodes re-derived),
# 1 -> 0 is on no path from 0 (tier 0)
RAISES = [(0, 0, 1, 2)] * 3 + [(1, 1830, 1831, 2), (0, 1, 0, 5)] + [(0, 0, 1, 2)] * 3
RAISE_INFO = np.array([3 | 3540 << 3] * 3 + [2 | 1740 << 3, 0] + [3 | 3540 << 3] * 3, dtype=np.uint32)


def raise_lists(ls):
    """RAISES as what_if_batch's metric lists: (link id, raising end, metric)."""
    by_ends = {frozenset((d[0], d[2])): lid for lid, d in ls.link_ids()}
    return [[(by_ends[frozenset((str(t), str(h)))], str(t), m)] for _, t, h, m in RAISES]


_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
import test_gpu_whatif_knobs as t
from helpers import row_digest
from openr_amd import host_backend

dbs, _ = t.bench_grid(60, 0)
als, _ = t.load_topology(host_backend(), dbs, [])
ls = als[t.A]._impl
if sys.argv[3] == "drain":
    idx = [k for k, _ in t.DRAINS]
    b = ls.what_if_batch(t.SRCS, idx, [[] for _ in idx], len(idx), drain=[[x] for _, x in t.DRAINS])
else:
    idx = [r[0] for r in t.RAISES]
    b = ls.what_if_batch(t.SRCS, idx, [[] for _ in idx], len(idx), metric=t.raise_lists(ls))
b.run()
b.sync()
np.savez(sys.argv[2], info=np.asarray(b.info(), dtype=np.uint32),
         digest=np.array([row_digest(*b.fetch(i)) for i in range(len(idx))], dtype=np.uint64))
"""


def _child(tmp_path, kind, **env):
    out = tmp_path / (kind + ".npz")
    subprocess.run([sys.executable, "-c", _CHILD, ROOT, str(out), kind], check=True,
                   env=dict(os.environ, **env), timeout=120)
    got = np.load(out)
    print(kind, env, "tiers", np.bincount(got["info"] & 7, minlength=5))
    return got["info"], got["digest"]


@pytest.fixture(scope="module")
def grid(hip, oracle, tmp_path_factory):
    """The oracle's row digest per distinct request of both jobs, and the info
    words of the drain job with no switch set."""
    dbs, _ = bench_grid(60, 0)
    als, _ = load_topology(hip, dbs, [])
    ls = als[A]._impl
    names = ls.node_names()
    nbrs = {s: ls.neighbors(s) for s in SRCS}
    oracles = Oracles(oracle, dbs)
    drains = {r: row_digest(*to_row(oracles([r[1]])._impl.run_spf_ignoring(SRCS[r[0]], []), names, nbrs[SRCS[r[0]]]))
              for r in set(DRAINS)}
    raise_oracles = RaiseOracles(oracle, dbs, dict(ls.link_ids()))
    raises = {}
    for r, met in zip(RAISES, raise_lists(ls)):
        if r not in raises:
            ref = raise_oracles([], met)._impl.run_spf_ignoring(SRCS[r[0]], [])
            raises[r] = row_digest(*to_row(ref, names, nbrs[SRCS[r[0]]]))
    info, digest = _child(tmp_path_factory.mktemp("default"), "drain")
    _check_digests(DRAINS, digest, drains)
    assert np.array_equal(info[BIG + [MID]], DEFAULT_INFO[BIG + [MID]])
    tier = info[36:36 + len(FAR)] & 7
    assert tier[FAR.index("3599")] == 0 and np.all(np.delete(tier, FAR.index("3599")) == 1)
    return drains, raises, info


def _check_digests(reqs, digest, want):
    """Every request's row is the oracle's for its kind (so repeated requests
    have equal rows)."""
    for i, r in enumerate(reqs):
        assert int(digest[i]) == want[r], (i, r)


def test_slot_tier_on_the_side_stream(grid, tmp_path):
    """ORH_WHATIF_T3_SPLIT=0: same rows, same tiers and affected counts as
    test_drain_tiers lists for the default run."""
    info, digest = _child(tmp_path, "drain", ORH_WHATIF_T3_SPLIT="0")
    _check_digests(DRAINS, digest, grid[0])
    assert np.array_equal(info, grid[2])
    assert set(int(x) for x in info & 7) == {0, 1, 2, 3}


def _check_full(info, default, keep_t2):
    tier, affected = info & 7, info >> 3
    small = (default & 7) <= 1  # the far-corner requests (tier 1, the corner itself 0) keep their info
    assert small.sum() == len(FAR) and np.array_equal(info[small], default[small])
    full = np.nonzero(tier == 4)[0]
    assert 1 <= len(full) <= 8
    assert set(full) <= set(BIG) | (set() if keep_t2 else {MID})
    rest = [i for i in BIG if tier[i] != 4]
    assert np.all(tier[rest] == 3) and np.all(affected[rest] == 3539)
    if keep_t2:
        assert tier[MID] == 2 and affected[MID] == 1739
    else:
        assert tier[MID] in (3, 4)  # tier 2 is skipped when full searches run
        assert tier[MID] == 4 or affected[MID] == 1739


def test_full_searches_skip_tier_2(grid, tmp_path):
    """ORH_WHATIF_FULL=8: tiers 0 and 1 as by default; 1 to 8 of the requests
    that outgrow tier 1 are searched in full (tier 4), the others, the lone
    tier-2 request among them, repaired in slots."""
    info, digest = _child(tmp_path, "drain", ORH_WHATIF_FULL="8")
    _check_digests(DRAINS, digest, grid[0])
    _check_full(info, grid[2], keep_t2=False)


def test_full_searches_behind_tier_2(grid, tmp_path):
    """ORH_WHATIF_FULL=8 ORH_WHATIF_SKIP_T2=0: request 35 is tier 2 again
    (1,739 affected); 1 to 8 of the 70 large requests are searched in full."""
    info, digest = _child(tmp_path, "drain", ORH_WHATIF_FULL="8", ORH_WHATIF_SKIP_T2="0")
    _check_digests(DRAINS, digest, grid[0])
    _check_full(info, grid[2], keep_t2=True)


def test_raises_take_no_full_search(grid, tmp_path):
    """ORH_WHATIF_FULL=8, a batch through orh_whatif_run_metrics whose raises
    take effect: no request is searched in full (the search knows no raised
    weights), tier 2 runs, and the tiers and counts are test_raise_tiers'."""
    info, digest = _child(tmp_path, "metric", ORH_WHATIF_FULL="8")
    _check_digests(RAISES, digest, grid[1])
    assert not np.any((info & 7) == 4)
    assert np.array_equal(info, RAISE_INFO)
