"""Reference model of a what-if impact record (orh_whatif_impact_rec in
include/openr_hip.h): plain numpy over one request's row and the base row of
its source.

Rows are indexed by node id: ``dist`` u32 with INF = unreached, ``nh`` one
first-hop mask word per node. A node unreached in the base row is in no class,
and neither is the source.
"""
import numpy as np

INF = 0xFFFFFFFF
NO_NODE = 0xFFFFFFFF
FIELDS = ("lost", "farther", "rehomed", "narrowed", "max_stretch", "worst_node", "sum_stretch",
          "lost_weight", "moved_weight")


def _popcount(a):
    a = np.ascontiguousarray(a, np.uint32)
    return np.unpackbits(a.view(np.uint8).reshape(-1, 4), axis=1).sum(axis=1)


def impact_classes(base_dist, base_nh, dist, nh, src):
    """Boolean arrays (lost, farther, rehomed, narrowed) and the int64 stretch
    (0 outside ``farther``) of every node."""
    bd, bn = np.asarray(base_dist, np.uint32), np.asarray(base_nh, np.uint32)
    rd, rn = np.asarray(dist, np.uint32), np.asarray(nh, np.uint32)
    live = bd != INF
    live[src] = False
    lost = live & (rd == INF)
    both = live & (rd != INF)
    farther = both & (rd != bd)
    rehomed = both & (rd == bd) & (rn != bn)
    narrowed = both & (_popcount(rn) < _popcount(bn))
    stretch = np.where(farther, rd.astype(np.int64) - bd.astype(np.int64), 0)
    return lost, farther, rehomed, narrowed, stretch


def impact_record(base_dist, base_nh, dist, nh, src, weight=None):
    """The record as a dict keyed by FIELDS (python ints)."""
    lost, farther, rehomed, narrowed, stretch = impact_classes(base_dist, base_nh, dist, nh, src)
    w = np.zeros(len(lost), np.uint64) if weight is None else np.asarray(weight, np.uint64)
    moved = lost | farther | rehomed
    any_farther = bool(farther.any())
    return {
        "lost": int(lost.sum()),
        "farther": int(farther.sum()),
        "rehomed": int(rehomed.sum()),
        "narrowed": int(narrowed.sum()),
        "max_stretch": int(stretch.max()) if any_farther else 0,
        # argmax returns the first maximum: the smallest node id on a tie
        "worst_node": int(np.argmax(stretch)) if any_farther else NO_NODE,
        "sum_stretch": int(stretch.sum()),
        "lost_weight": int(w[lost].sum(dtype=np.uint64)),
        "moved_weight": int(w[moved].sum(dtype=np.uint64)),
    }


def node_counts(classes):
    """(lost, moved) per node over an iterable of impact_classes results."""
    lost = moved = None
    for lo, fa, re, _, _ in classes:
        if lost is None:
            lost, moved = np.zeros(len(lo), np.uint32), np.zeros(len(lo), np.uint32)
        lost += lo
        moved += lo | fa | re
    return lost, moved
