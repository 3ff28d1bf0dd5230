"""Reference model of a two-sided what-if record (orh_whatif_gain_rec in
include/openr_hip.h): plain numpy over one request's row and the base row of
its source, in the style of tests/impact_model.py.

Rows are indexed by node id: ``dist`` u32 with INF = unreached, ``nh`` one
first-hop mask word per node. A node unreached in the base row is in no class,
and neither is the source.
"""
import collections

import numpy as np

from impact_model import INF, NO_NODE, _popcount

FIELDS = ("lost", "farther", "nearer", "rehomed", "narrowed", "widened", "max_stretch", "worst_node", "max_gain",
          "best_node", "sum_stretch", "sum_gain", "lost_weight", "moved_weight", "nearer_weight")
U64_FIELDS = ("sum_stretch", "sum_gain", "lost_weight", "moved_weight", "nearer_weight")
# the fields orh_whatif_impact_rec has too; equal on rows without a nearer node
SHARED = ("lost", "farther", "rehomed", "narrowed", "max_stretch", "worst_node", "sum_stretch", "lost_weight",
          "moved_weight")
# orh_whatif_gain_rec, byte for byte
REC = np.dtype([(f, "<u8" if f in U64_FIELDS else "<u4") for f in FIELDS])

Classes = collections.namedtuple("Classes", "lost farther nearer rehomed narrowed widened stretch gain")


def gain_classes(base_dist, base_nh, dist, nh, src):
    """Boolean arrays per class, and the int64 stretch (0 outside ``farther``)
    and gain (0 outside ``nearer``) of every node."""
    bd, bn = np.asarray(base_dist, np.uint32), np.asarray(base_nh, np.uint32)
    rd, rn = np.asarray(dist, np.uint32), np.asarray(nh, np.uint32)
    live = bd != INF
    live[src] = False
    lost = live & (rd == INF)
    both = live & (rd != INF)
    farther = both & (rd > bd)
    nearer = both & (rd < bd)
    rehomed = both & (rd == bd) & (rn != bn)
    narrowed = both & (_popcount(rn) < _popcount(bn))
    widened = both & (_popcount(rn) > _popcount(bn))
    diff = rd.astype(np.int64) - bd.astype(np.int64)
    return Classes(lost, farther, nearer, rehomed, narrowed, widened, np.where(farther, diff, 0),
                   np.where(nearer, -diff, 0))


def moved(c):
    return c.lost | c.farther | c.nearer | c.rehomed


def record_of(c, weight=None):
    """The record of one gain_classes result as a dict keyed by FIELDS (python ints)."""
    w = np.zeros(len(c.lost), np.uint64) if weight is None else np.asarray(weight, np.uint64)
    far, near = bool(c.farther.any()), bool(c.nearer.any())
    return {
        "lost": int(c.lost.sum()),
        "farther": int(c.farther.sum()),
        "nearer": int(c.nearer.sum()),
        "rehomed": int(c.rehomed.sum()),
        "narrowed": int(c.narrowed.sum()),
        "widened": int(c.widened.sum()),
        "max_stretch": int(c.stretch.max()) if far else 0,
        # argmax returns the first maximum: the smallest node id on a tie
        "worst_node": int(np.argmax(c.stretch)) if far else NO_NODE,
        "max_gain": int(c.gain.max()) if near else 0,
        "best_node": int(np.argmax(c.gain)) if near else NO_NODE,
        "sum_stretch": int(c.stretch.sum()),
        "sum_gain": int(c.gain.sum()),
        "lost_weight": int(w[c.lost].sum(dtype=np.uint64)),
        "moved_weight": int(w[moved(c)].sum(dtype=np.uint64)),
        "nearer_weight": int(w[c.nearer].sum(dtype=np.uint64)),
    }


def gain_record(base_dist, base_nh, dist, nh, src, weight=None):
    return record_of(gain_classes(base_dist, base_nh, dist, nh, src), weight)


def records_of(classes, weight=None):
    """Model records of many requests: a dict of arrays keyed by FIELDS, with
    the dtypes of the record."""
    recs = [record_of(c, weight) for c in classes]
    return {f: np.array([r[f] for r in recs], REC[f]) for f in FIELDS}


def node_counts(classes):
    """(lost, moved, nearer) per node over an iterable of gain_classes results."""
    out = None
    for c in classes:
        if out is None:
            out = [np.zeros(len(c.lost), np.uint32) for _ in range(3)]
        out[0] += c.lost
        out[1] += moved(c)
        out[2] += c.nearer
    return tuple(out)


def zero_record():
    """The record of a request whose row equals the base row (tier 0)."""
    return {f: NO_NODE if f in ("worst_node", "best_node") else 0 for f in FIELDS}
