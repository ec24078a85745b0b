"""Shared by tests/test_delta_log_model.py (CPU) and tests/test_gpu_delta_log.py:
delta_log_ref, the expectation of crdt_awset_delta_join_log_async /
crdt_awset_delta_exchange_log_async (include/crdtgpu.h), and the case sets both
files draw from.

delta_log_ref(a, b) is delta_pair_ref(a, b) of tests/delta_pair_cases.py (the C
oracle's delta fold of one source per document, and the kinds) and then log_of of
tests/join_log_cases.py per direction: diff_doc on (dst, the oracle's output),
document by document, laid out as the call lays it out.  Nothing in it comes from
the code under test.

A replica's documents are lists docs[d] = (entries, tombstones, vv); counters stay
within 0..MAX_C so that tests/counter_maps.py can push the same cases up to the
64-bit edges.
"""

import numpy as np

from crdtgpu import CRDT_DELTA_DELTA
from delta_pair_cases import (FEATURES as PAIR_FEATURES, MAX_C, _doc_lists, delta_pair_ref, doc_features, edge_pair,
                              has_dot, on_wave_path, phase2_doc, random_pair)
from join_log_cases import LogRef, _slots_idx, log_of
from sources_cases import make_replica

U8, U32, U64 = np.uint8, np.uint32, np.uint64
LOG_FEATURES = ("p1_update_p2_remove", "tomb_removes_dst_only", "delta_keeps_covered_dst_only", "none_src_ahead",
                "tomb_absent_key")
ALL_FEATURES = LOG_FEATURES + ("p1_add_p2_remove", "tomb_readded")
assert set(ALL_FEATURES) == set(LOG_FEATURES) | set(PAIR_FEATURES)
PAD = 70  # keys added on both sides to take a feature document to the block path


# ------------------------------------------------------------------ reference

class DeltaLogRef:
    """pair: the PairRef (oracle outputs ab / ba, kinds, statuses); ab / ba: a LogRef per
    direction whose .out is the oracle's fold output (packed at its own offsets: compare
    it per document, delta_pair_cases.assert_direction) and whose .log is laid out as the
    call lays it out."""

    def __init__(self, pair, ab, ba):
        self.pair, self.ab, self.ba = pair, ab, ba


def _log_ref(rc, dst, src, out):
    log = log_of(dst, src, out.as_batch())
    return LogRef(rc, out, log, _slots_idx(log["rem_offsets"], log["rem_counts"]),
                  _slots_idx(log["ups_offsets"], log["ups_counts"]))


def delta_log_ref(a, b):
    a, b = a.numpy(), b.numpy()
    pr = delta_pair_ref(a, b)
    return DeltaLogRef(pr, _log_ref(pr.rc_ab, a.state, b.state, pr.ab), _log_ref(pr.rc_ba, b.state, a.state, pr.ba))


# ------------------------------------------------------------------- features

def log_features(d_entries, dvv, svv, R, s_actor, s_entries, s_tombs):
    """(kind, the ALL_FEATURES the direction dst <- src of one document exercises)."""
    kind, f = doc_features(d_entries, dvv, svv, R, s_actor, s_entries, s_tombs)
    if kind != CRDT_DELTA_DELTA:
        return kind, f
    own = {k: (a, c) for k, a, c in s_entries}
    have = {k: (a, c) for k, a, c in d_entries}
    dropped = set()  # keys an effective tombstone D has not seen removes in phase 2
    for k, a, c in s_tombs:
        if k in own and (own[k][0] != a or own[k][1] > c):
            continue
        if not has_dot(dvv, R, a, c):
            dropped.add(k)
    for k in dropped:
        if k in have and k in own and not has_dot(dvv, R, *own[k]):
            f.add("p1_update_p2_remove")
        if k in have and k not in own:
            f.add("tomb_removes_dst_only")
    for k, (a, c) in have.items():
        if k not in own and k not in dropped and has_dot(svv, R, a, c):
            f.add("delta_keeps_covered_dst_only")
    return kind, f


def feature_docs(R=2, kmul=1):
    """name -> ((entries, tombstones, vv) of a, the same of b): one deterministic document
    per LOG_FEATURES whose direction a <- b (a's actor 0, b's actor s = 1 % R) shows it.
    a's clock has met s (a[s] = 4) and has not seen s's dots above 4."""
    s = 1 % R
    va, vb = [3] * R, [8] * R
    va[s] = 4
    K = lambda k: k * kmul  # noqa: E731
    docs = {}
    # a holds 40 under (s, 2); b holds it under (s, 7), which a has not seen (phase 1 moves the
    # key there), and a tombstone (s, 8) of it that the filter lets through and a has not seen
    docs["p1_update_p2_remove"] = (([(K(10), 0, 2), (K(40), s, 2)], [], list(va)),
                                   ([(K(10), 0, 2), (K(40), s, 7)], [(K(40), s, 8)], list(vb)))
    # a alone holds 50; b's tombstone of it carries a dot a has not seen
    docs["tomb_removes_dst_only"] = (([(K(10), 0, 2), (K(50), 0, 1)], [], list(va)),
                                     ([(K(10), 0, 2)], [(K(50), s, 6)], list(vb)))
    # a alone holds 60 under a dot b's clock covers: FULL would remove it, DELTA keeps it;
    # b's 70 under an unseen dot makes the document DELTA
    docs["delta_keeps_covered_dst_only"] = (([(K(10), 0, 2), (K(60), 0, 3)], [], list(va)),
                                            ([(K(10), 0, 2), (K(70), s, 6)], [], list(vb)))
    # nothing of b is new to a, but b's clock is ahead in component 0: NONE, a's clock stays
    ahead = list(va)
    ahead[0] = 9
    docs["none_src_ahead"] = (([(K(10), 0, 2)], [], list(va)), ([(K(10), 0, 2)], [], ahead))
    # b's only news is a tombstone of a key neither side holds: DELTA, no record, the clock moves
    docs["tomb_absent_key"] = (([(K(10), 0, 2)], [], list(va)), ([(K(10), 0, 2)], [(K(99), s, 8)], list(vb)))
    return docs


def at_block_size(x, y, kmul=1):
    """The document with PAD further keys on both sides, under a dot both clocks have seen."""
    pad = [(kmul * (1000 + 3 * i), 0, 1) for i in range(PAD)]
    return (x[0] + pad, x[1], x[2]), (y[0] + pad, y[1], y[2])


def feature_list(R=2):
    """[(name, size, doc of a, doc of b)]: every ALL_FEATURES document at wave and at block
    size (the phase-2 document of delta_pair_cases shows p1_add_p2_remove and tomb_readded)."""
    out = []
    docs = dict(feature_docs(R))
    docs["phase2"] = phase2_doc(R)
    for name, (x, y) in docs.items():
        out.append((name, "wave", x, y))
        bx, by = at_block_size(x, y)
        out.append((name, "block", bx, by))
    return out


def feature_pair(R=2, **lay):
    fl = feature_list(R)
    return make_replica(R, [f[2] for f in fl], actor=0, **lay), make_replica(R, [f[3] for f in fl], actor=1 % R, **lay)


def edge_log_pair(R=2, big=True):
    """edge_pair's dispatch edges followed by every feature document."""
    da, db = edge_pair(R, big=big)
    fl = feature_list(R)
    da += [f[2] for f in fl]
    db += [f[3] for f in fl]
    return make_replica(R, da, actor=0), make_replica(R, db, actor=1 % R)


RANDOM_DOCS = 300


def case_sets():
    """name -> (a, b): the sets both test files run (host Replicas)."""
    sets = {"edges": edge_log_pair(), "features": feature_pair()}
    for R in (1, 2, 5, 64):
        sets["random%d" % R] = random_pair(8000 + R, RANDOM_DOCS, R)
    return sets


def census(a, b):
    """{(path, direction, kind)}, {(path, feature)} over the documents of a pair."""
    kinds, feats = set(), set()
    R = a.state.R
    for d in range(a.n_docs):
        path = "wave" if on_wave_path(a, b, d) else "block"
        ea, ta, va, aa = _doc_lists(a, d)
        eb, tb, vb, ab = _doc_lists(b, d)
        k, f = log_features(ea, va, vb, R, ab, eb, tb)
        kinds.add((path, "ab", k))
        feats |= {(path, x) for x in f}
        k, f = log_features(eb, vb, va, R, aa, ea, ta)
        kinds.add((path, "ba", k))
        feats |= {(path, x) for x in f}
    return kinds, feats
