"""Shared by tests/test_delta_pair_model.py (CPU) and tests/test_gpu_delta_pair.py:
delta_pair_ref, the expectation of crdt_awset_delta_join_async /
crdt_awset_delta_exchange_async (include/crdtgpu.h), and the case sets both files
draw from.

delta_pair_ref(a, b) is the C oracle's delta fold of one source per document --
oracle.fold(CRDT_FOLD_DELTA, a.state, sources_ref([b])) and the mirror -- so it is
compared per document (the fold packs its output at other offsets than the
join's layout), plus the kind of every document recomputed here from the inputs.

A replica's documents are lists docs[d] = (entries, tombstones, vv) as in
tests/sources_cases.py; counters stay within 0..9 so that tests/counter_maps.py
can push the same cases up to the 64-bit edges.
"""

import random

import numpy as np

from crdtgpu import CRDT_DELTA_DELTA, CRDT_DELTA_FULL, CRDT_DELTA_NONE, CRDT_FOLD_DELTA
from helpers import out_doc
from oracle import oracle
from sources_cases import make_replica, sources_ref

U32, U64 = np.uint32, np.uint64
MAX_C = 9        # counters and clock values of every case here lie in 0..MAX_C
WAVE_MAX = 64    # kPairWaveMax: live entries, and tombstones, per side on the wave path
PAIR_WAVES = 4   # kPairWaves: documents per workgroup of the wave path
BLOCK_WINDOW = 1024  # kPairBlockNT * kPairBlockIPT: merged positions per step of the block path
KINDS = (CRDT_DELTA_NONE, CRDT_DELTA_DELTA, CRDT_DELTA_FULL)
FEATURES = ("p1_add_p2_remove", "tomb_readded", "tomb_absent_key", "none_src_ahead")


# ------------------------------------------------------------------ reference

class PairRef:
    """ab / ba: the oracle's fold outputs (a <- b, b <- a); kind_ab / kind_ba: u8 per
    document; rc_ab / rc_ba: the oracle's status (CRDT_E_ACTOR_RANGE or 0)."""

    def __init__(self, ab, ba, kind_ab, kind_ba, rc_ab, rc_ba):
        self.ab, self.ba, self.kind_ab, self.kind_ba, self.rc_ab, self.rc_ba = ab, ba, kind_ab, kind_ba, rc_ab, rc_ba


def _doc_lists(rep, d):
    """(entries, tombstones, vv, actor) of document d of a host Replica, live prefixes only."""
    e, vv = rep.state.doc(d)
    t = rep.tombs.doc(d) if rep.tombs is not None else []
    actor = int(rep.doc_actor[d]) if rep.doc_actor is not None else rep.actor
    return e, t, vv, actor


def has_dot(vv, R, actor, counter):
    return actor < R and vv[actor] >= counter


def doc_kind(dvv, R, s_actor, s_entries, s_tombs):
    """The kind of one direction of one document (awset-delta_test.go:51-65, 79-105);
    dst's entries play no part in it."""
    if (dvv[s_actor] if s_actor < R else 0) == 0:
        return CRDT_DELTA_FULL
    own = {k: (a, c) for k, a, c in s_entries}
    changed = any(not has_dot(dvv, R, a, c) for _, a, c in s_entries)
    deleted = any(not (k in own and (own[k][0] != a or own[k][1] > c)) for k, a, c in s_tombs)
    return CRDT_DELTA_DELTA if changed or deleted else CRDT_DELTA_NONE


def doc_features(d_entries, dvv, svv, R, s_actor, s_entries, s_tombs):
    """Which of FEATURES the direction dst <- src of one document exercises."""
    kind = doc_kind(dvv, R, s_actor, s_entries, s_tombs)
    f = set()
    if kind == CRDT_DELTA_NONE and any(s > v for s, v in zip(svv, dvv)):
        f.add("none_src_ahead")
    if kind != CRDT_DELTA_DELTA:
        return kind, f
    own = {k: (a, c) for k, a, c in s_entries}
    have = {k for k, _, _ in d_entries}
    added = {k for k, a, c in s_entries if k not in have and not has_dot(dvv, R, a, c)}
    for k, a, c in s_tombs:
        if k in own and (own[k][0] != a or own[k][1] > c):
            f.add("tomb_readded")
            continue
        if k not in have and k not in own:
            f.add("tomb_absent_key")
        if k in added and not has_dot(dvv, R, a, c):
            f.add("p1_add_p2_remove")
    return kind, f


def kinds_of(dst, src):
    """u8 per document: the kind of dst <- src (host Replicas; dst's tombstones unused)."""
    n, R = dst.n_docs, dst.state.R
    vv = np.asarray(dst.state.vv, U64)[: n * R].reshape(n, R)
    out = np.zeros(n, np.uint8)
    for d in range(n):
        e, t, _, actor = _doc_lists(src, d)
        out[d] = doc_kind(vv[d].tolist(), R, actor, e, t)
    return out


def delta_pair_ref(a, b):
    rc_ab, ab = oracle.fold(CRDT_FOLD_DELTA, a.state, sources_ref([b]).msg)
    rc_ba, ba = oracle.fold(CRDT_FOLD_DELTA, b.state, sources_ref([a]).msg)
    return PairRef(ab, ba, kinds_of(a, b), kinds_of(b, a), rc_ab, rc_ba)


def assert_direction(got, want, a_state, b_state, what=""):
    """got: a host output in the join's layout; want: the oracle's fold output.  Every
    document's entries, count and clock equal; the slot bounds are the join's."""
    n, R = a_state.n_docs, a_state.R
    ao, bo = np.asarray(a_state.offsets, U32).astype(np.int64), np.asarray(b_state.offsets, U32).astype(np.int64)
    assert (np.asarray(got.offsets, U32)[: n + 1].astype(np.int64) == (ao + bo) % (1 << 32)).all(), what + " offsets"
    assert (np.asarray(got.counts, U32)[:n] == np.asarray(want.counts, U32)[:n]).all(), what + " counts"
    for d in range(n):
        g, w = out_doc(got, d, R), out_doc(want, d, R)
        assert g == w, "%s document %d: got %r, expected %r" % (what, d, g, w)


# ------------------------------------------------------------------- builders

def seq_keys(n, start=1, step=3):
    return [start + step * i for i in range(n)]


def pair_docs(rng, R, na, nb, nta, ntb, mode, actor_a=0, actor_b=None, kmul=1):
    """One document of both replicas: ((entries, tombstones, vv) of a, the same of b).
    na / nb entries, nta / ntb tombstones, counters in 1..MAX_C - 1.
    mode 0: neither clock has met the other's actor (FULL both ways);
    mode 1: clocks at random above 0 (mostly DELTA);
    mode 2: each clock covers every dot of the other side and every tombstone is
            re-added where the entries allow it (NONE), each clock ahead of the
            other in one component when R >= 2."""
    actor_b = (1 % R) if actor_b is None else actor_b
    hi = MAX_C - 1
    U = max(na, nb) + (min(na, nb) + 1) // 2 + 2
    universe = [kmul * k for k in seq_keys(U)]
    ka = sorted(rng.sample(universe, na))
    kb = sorted(rng.sample(universe, nb))
    ea = [(k, rng.randrange(R), rng.randint(2, hi)) for k in ka]
    da = {k: (a, c) for k, a, c in ea}
    eb = [(k,) + (da[k] if k in da and rng.random() < 0.5 else (rng.randrange(R), rng.randint(2, hi))) for k in kb]

    def tombs(own, other, nt):
        if nt == 0:
            return []
        od = {k: (a, c) for k, a, c in own}
        absent = [kmul * (U * 3 + 5 + 3 * i) + 1 for i in range(nt)]  # keys of neither replica
        if mode == 2:
            pool = [k for k, _, _ in own][:nt]
            pool += absent[: nt - len(pool)]
        else:
            cand = sorted(set(universe) | set(absent[: max(2, nt // 4)]))
            pool = rng.sample(cand, nt) if nt <= len(cand) else cand + absent[len(absent) - (nt - len(cand)):]
        out = []
        for k in sorted(set(pool)):
            if k in od and (mode == 2 or rng.random() < 0.5):  # re-added since: kept back by the filter
                a, c = od[k]
                out.append((k, (a + 1) % R, rng.randint(1, hi)) if R > 1 and rng.random() < 0.5 else (k, a, c - 1))
            elif k in od:  # still deleted as far as the filter can tell
                a, c = od[k]
                out.append((k, a, rng.randint(c, MAX_C)))
            else:
                out.append((k, rng.randrange(R), rng.randint(1, MAX_C)))
        return out

    ta, tb = tombs(ea, eb, nta), tombs(eb, ea, ntb)
    if mode == 0:
        va, vb = [rng.randint(0, MAX_C) for _ in range(R)], [rng.randint(0, MAX_C) for _ in range(R)]
        va[actor_b] = 0
        vb[actor_a] = 0
    elif mode == 1:
        va, vb = [rng.randint(1, MAX_C) for _ in range(R)], [rng.randint(1, MAX_C) for _ in range(R)]
    else:
        va, vb = [hi] * R, [hi] * R
        va[0] = MAX_C
        vb[(R - 1) if R > 1 else 0] = MAX_C
    return (ea, ta, va), (eb, tb, vb)


def phase2_doc(R, kmul=1):
    """A document whose a <- b adds key 40 in phase 1 and removes it in phase 2: b holds
    it with a dot a has not seen, and a tombstone of it that the filter lets through
    (same actor, counter not below the entry's) and a has not seen either.  b also
    holds a re-added key (70) and a tombstone of a key neither side has (99)."""
    s = 1 % R
    ea = [(10 * kmul, 0, 2), (70 * kmul, 0, 1)]
    eb = [(10 * kmul, 0, 2), (40 * kmul, s, 7), (70 * kmul, s, 6)]
    tb = [(40 * kmul, s, 8), (70 * kmul, s, 5), (99 * kmul, s, 8)]
    va, vb = [3] * R, [8] * R
    va[s] = 4 if R > 1 else 3
    return (ea, [], va), (eb, tb, vb)


def build_pair(R, docs_a, docs_b, lay_a=None, lay_b=None, actor_a=0, actor_b=None, **kw):
    """Host Replicas (a, b) of the documents; lay_*: make_replica's layout arguments."""
    actor_b = (1 % R) if actor_b is None else actor_b
    a = make_replica(R, docs_a, actor=actor_a, **(lay_a or {}), **kw)
    b = make_replica(R, docs_b, actor=actor_b, **(lay_b or {}), **kw)
    return a, b


def random_pair(seed, n_docs, R, max_e=10, max_t=4, lay_a=None, lay_b=None, tombs_a=True, tombs_b=True,
                doc_actors=False):
    """n_docs small documents, the modes of pair_docs in turn, every 13th the
    phase-2 document.  doc_actors: both replicas name their actor per document."""
    rng = random.Random(seed)
    da, db = [], []
    acts_a = [rng.randrange(R) for _ in range(n_docs)] if doc_actors else None
    acts_b = [rng.randrange(R) for _ in range(n_docs)] if doc_actors else None
    for d in range(n_docs):
        aa = acts_a[d] if doc_actors else 0
        ab = acts_b[d] if doc_actors else 1 % R
        if d % 13 == 6 and not doc_actors:
            x, y = phase2_doc(R)
        else:
            x, y = pair_docs(rng, R, rng.randint(0, max_e), rng.randint(0, max_e), rng.randint(0, max_t),
                             rng.randint(0, max_t), d % 3, aa, ab)
        da.append(x)
        db.append(y)
    a = make_replica(R, da, actor=0, doc_actor=acts_a, tombs=tombs_a, **(lay_a or {}))
    b = make_replica(R, db, actor=1 % R, doc_actor=acts_b, tombs=tombs_b, **(lay_b or {}))
    return a, b


EDGE_SIZES = (0, 1, 63, 64, 65, 129)
EDGE_TOMBS = (0, 1, 64, 65)
LOOP_ENTRIES = 3000  # one document of this many entries a side: the block path steps its window


def edge_pair(R=2, seed=4100, big=True):
    """Deterministic sizes around the dispatch edge, every combination that changes the
    path: all EDGE_SIZES x EDGE_SIZES without tombstones, EDGE_TOMBS x EDGE_TOMBS on
    three entry shapes, each in the three modes of pair_docs; the phase-2 document
    at wave and at block size; with big, one document of LOOP_ENTRIES a side."""
    rng = random.Random(seed)
    shapes = [(na, nb, 0, 0) for na in EDGE_SIZES for nb in EDGE_SIZES]
    shapes += [(na, nb, ta, tb) for na, nb in ((1, 1), (64, 64), (63, 65), (129, 1)) for ta in EDGE_TOMBS
               for tb in EDGE_TOMBS]
    da, db = [], []
    for i, (na, nb, ta, tb) in enumerate(shapes):
        for mode in range(3):
            x, y = pair_docs(rng, R, na, nb, ta, tb, mode, kmul=(1 if i % 2 else 2 ** 40 + 7))
            da.append(x)
            db.append(y)
    x, y = phase2_doc(R)
    da.append(x)
    db.append(y)
    # the same at block size: 70 further keys on both sides, unseen dots on neither
    pad = [(1000 + 3 * i, 0, 1) for i in range(70)]
    da.append((x[0] + pad, x[1], x[2]))
    db.append((y[0] + pad, y[1], y[2]))
    if big:
        for mode in (1, 2, 0):
            x, y = pair_docs(rng, R, LOOP_ENTRIES, LOOP_ENTRIES - 77, 5, 70, mode)
            da.append(x)
            db.append(y)
    return da, db


def on_wave_path(a, b, d):
    ea, ta, _, _ = _doc_lists(a, d)
    eb, tb, _, _ = _doc_lists(b, d)
    return max(len(ea), len(eb), len(ta), len(tb)) <= WAVE_MAX


def census(a, b):
    """{(path, direction, kind)}, {(path, feature)} over the documents of a pair."""
    kinds, feats = set(), set()
    R = a.state.R
    for d in range(a.n_docs):
        path = "wave" if on_wave_path(a, b, d) else "block"
        ea, ta, va, aa = _doc_lists(a, d)
        eb, tb, vb, ab = _doc_lists(b, d)
        k, f = doc_features(ea, va, vb, R, ab, eb, tb)
        kinds.add((path, "ab", k))
        feats |= {(path, x) for x in f}
        k, f = doc_features(eb, vb, va, R, aa, ea, ta)
        kinds.add((path, "ba", k))
        feats |= {(path, x) for x in f}
    return kinds, feats


def replica_of_ref(states, ids, R, actor, **lay):
    """Map-based AWSetDelta states (oracle/awset_ref.py), one per document -> a host Replica."""
    from helpers import ents, pad

    docs = [(ents(s.Entries, ids), ents(s.Deleted, ids), pad(s.VersionVector, R)) for s in states]
    return make_replica(R, docs, actor=actor, **lay)
