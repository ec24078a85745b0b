"""Shared by tests/test_replica_inplace_model.py (CPU) and
tests/test_gpu_replica_inplace.py: the deterministic case table of
crdt_replica_scatter_inplace_async (include/crdtgpu.h).  No RNG decides an edge:
every size below is written out, and random generators only fill documents whose
sizes do not matter.

A case is (rep, sub, idx, n_idx): host Replicas (rep with counts, since a
document's length changes), a u32 index array and an int or None.  The kernels
work in these units (csrc/replica_inplace.hip), and the cases are sized around
them:
  kInpScanChunk   = 1,024 sub documents per workgroup of the spill scan,
  kInpPartStep    = 1,024 partial sums per step of the one-workgroup partials scan,
  kInpGatherChunk = 2,048 positions of sub's slot space per gather step,
  kInpRun         = 1,024 documents of a gather chunk staged in LDS at most.
"""

import random

import numpy as np

from crdtgpu.batch import AWSetBatch, Replica, TombBatch
from sources_cases import make_replica, rand_replicas, tiny_replicas
from test_replica_model import edge_docs, seq_list

U32, U64 = np.uint32, np.uint64
ONES32 = 2 ** 32 - 1
K_SCAN, K_PART, K_GATHER, K_RUN = 1024, 1024, 2048, 1024

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def pack_caps(lists, caps, garbage=None, lead=0):
    """[(key, actor, counter)] per document -> (offsets, counts, keys, actors, counters)
    with caps[d] slots for document d (>= its length) and `lead` unused slots before
    the first; slack filled from the numpy rng `garbage` (stale, non-zero) when given."""
    n = len(lists)
    counts = np.array([len(x) for x in lists], U32)
    caps = np.asarray(caps, np.int64)
    assert len(caps) == n and (caps >= counts).all()
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(caps, out=offsets[1:])
    offsets += lead
    m = max(int(offsets[-1]), 1)
    if garbage is not None:
        keys = garbage.integers(1, 2 ** 63, m, dtype=np.int64).view(U64).copy()
        actors = garbage.integers(1, 2 ** 31, m, dtype=np.int64).astype(U32)
        counters = garbage.integers(1, 2 ** 63, m, dtype=np.int64).view(U64).copy()
    else:
        keys, actors, counters = np.zeros(m, U64), np.zeros(m, U32), np.zeros(m, U64)
    for d, x in enumerate(lists):
        o = int(offsets[d])
        for i, (k, a, c) in enumerate(x):
            keys[o + i], actors[o + i], counters[o + i] = k, a, c
    return offsets.astype(U32), counts, keys, actors, counters


def make_target(R, docs, ecaps, tcaps=None, doc_actor=None, garbage=None, lead=0, actor=0):
    """docs[d] = (entries, tombstones, vv) laid out with ecaps[d] entry slots and
    tcaps[d] tombstone slots (tcaps None: the replica keeps no Deleted)."""
    o, c, k, a, n_ = pack_caps([d[0] for d in docs], ecaps, garbage, lead)
    vv = np.array([d[2] for d in docs], U64).reshape(-1)
    tb = None
    if tcaps is not None:
        to, tc, tk, ta, tn = pack_caps([d[1] for d in docs], tcaps, garbage, lead)
        tb = TombBatch(to, tk, ta, tn, counts=tc)
    return Replica(AWSetBatch(R, o, k, a, n_, vv, counts=c), tb, actor,
                   None if doc_actor is None else np.asarray(doc_actor, U32))


def _doc(d, ne, nt, R=3, salt=0):
    return (seq_list(100 * d + salt, ne, R), seq_list(100 * d + 50 + salt, nt, R), [d + 1 + salt] * R)


def _simple(n_rep, ecap, tcap, sub_sizes, idx, n_idx=None, R=3):
    """n_rep documents of 2 entries and 1 tombstone in ecap / tcap slots; sub documents
    of sub_sizes[j] = (ne, nt) entries and tombstones in exactly that many slots."""
    g = np.random.default_rng(11)
    rep = make_target(R, [_doc(d, min(2, ecap), min(1, tcap), R) for d in range(n_rep)], [ecap] * n_rep, [tcap] * n_rep,
                      doc_actor=[d % R for d in range(n_rep)], garbage=g)
    sub = make_replica(R, [_doc(j, ne, nt, R, salt=7) for j, (ne, nt) in enumerate(sub_sizes)], with_counts=True,
                       actor=1, doc_actor=[(j + 1) % R for j in range(len(sub_sizes))])
    return rep, sub, np.asarray(idx, U32), n_idx


def _with_counts(r):
    """r with explicit counts on the state and the tombstones (as a target needs them)."""
    s, t = r.state, r.tombs
    sc = s.counts if s.counts is not None else np.diff(s.offsets.astype(np.int64)).astype(U32)
    st = AWSetBatch(s.R, s.offsets, s.keys, s.actors, s.counters, s.vv, counts=sc)
    if t is not None:
        tc = t.counts if t.counts is not None else np.diff(t.offsets.astype(np.int64)).astype(U32)
        t = TombBatch(t.offsets, t.keys, t.actors, t.counters, counts=tc)
    return Replica(st, t, r.actor, r.doc_actor)


def _gather_case(lead_sub, lead_rep):
    """sub = edge_docs() in exactly their sizes (documents end at sub positions 2,047 /
    2,048 / 2,049 past the lead, one spans three chunks, 3,000 documents of 0 or 1
    entries share chunks); the target's document idx[j] has one slot more than sub
    document j needs when j % 3 != 0, one fewer otherwise, and slots for both
    parities of the destination."""
    docs = edge_docs()
    m = len(docs)
    sub = make_replica(2, docs, with_counts=True, actor=1, lead=lead_sub, garbage=np.random.default_rng(5))
    n = m + 40
    perm = [(7 * j + 3) % n for j in range(m)]  # 7 and n = 3,350 are coprime: no document twice
    ecaps, tcaps = [2] * n, [1] * n
    for j, d in enumerate(perm):
        ne, nt = len(docs[j][0]), len(docs[j][1])
        ecaps[d] = ne + 1 if j % 3 else max(ne - 1, 0)
        tcaps[d] = nt + (j % 2)
    rep_docs = [(seq_list(3 * d, min(ecaps[d], 2), 2), seq_list(3 * d + 1, min(tcaps[d], 1), 2), [9, d]) for d in range(n)]
    rep = make_target(2, rep_docs, ecaps, tcaps, garbage=np.random.default_rng(6), lead=lead_rep)
    return rep, sub, np.array(perm, U32), None


def _scan_case(m, spill):
    """m sub documents of one entry and one tombstone onto m + 5 target documents,
    descending; the target's entry slots decide who spills."""
    n = m + 5
    idx = np.arange(n - 1, n - 1 - m, -1).astype(U32)
    cap = np.ones(n, np.int64)
    if spill == "one":
        cap[idx[m // 2]] = 0
    elif spill == "all":
        cap[:] = 0
    elif spill == "alternate":
        cap[idx[::2]] = 0
    off = np.zeros(n + 1, U32)
    np.cumsum(cap, out=off[1:])
    tot = max(int(off[-1]), 1)
    toff = np.arange(n + 1, dtype=U32)
    rep = Replica(AWSetBatch(2, off, np.arange(tot, dtype=U64) + U64(5), np.zeros(tot, U32), np.ones(tot, U64),
                             np.arange(2 * n, dtype=U64), counts=cap.astype(U32)),
                  TombBatch(toff, np.arange(n, dtype=U64), np.zeros(n, U32), np.ones(n, U64), counts=np.ones(n, U32)), 0)
    one = np.arange(m + 1, dtype=U32)
    sub = Replica(AWSetBatch(2, one, np.arange(m, dtype=U64) * U64(3) + U64(1000), np.ones(m, U32), np.full(m, 7, U64),
                             np.arange(2 * m, dtype=U64) + U64(10 ** 6), counts=np.ones(m, U32)),
                  TombBatch(one, np.arange(m, dtype=U64) + U64(2000), np.ones(m, U32), np.full(m, 8, U64),
                            counts=np.ones(m, U32)), 1)
    return rep, sub, idx, None


def cases():
    """name -> (rep, sub, idx, n_idx) of every small case."""
    def make():
        out = {}
        # --- fit verdicts: sub document j -> target document idx[j]; (ce, ct) against (ne, nt)
        fits = [("eq", 5, 2, 5, 1), ("plus1", 5, 2, 6, 1), ("empty", 5, 2, 0, 0), ("zero-cap-0", 0, 0, 0, 0),
                ("zero-cap-1", 0, 0, 1, 0), ("entries-fit-tombs-not", 8, 1, 3, 2), ("tombs-fit-entries-not", 2, 4, 3, 1),
                ("tombs-eq", 4, 3, 2, 3)]
        n = 2 * len(fits) + 1
        idx = [2 * k + 1 for k in range(len(fits))][::-1]
        ecaps, tcaps = [3] * n, [2] * n
        for (_, ce, ct, _, _), d in zip(fits, idx):
            ecaps[d], tcaps[d] = ce, ct
        g = np.random.default_rng(21)
        rep = make_target(3, [_doc(d, min(ecaps[d], 2), min(tcaps[d], 1)) for d in range(n)], ecaps, tcaps,
                          doc_actor=[d % 3 for d in range(n)], garbage=g, lead=1)
        sub = make_replica(3, [_doc(j, ne, nt, salt=7) for j, (_, _, _, ne, nt) in enumerate(fits)], slack=2,
                           with_counts=True, garbage=g, actor=2)
        out["fit-edges"] = (rep, sub, np.array(idx, U32), None)
        # --- replica forms at R = 1, 3, 64
        for R in (1, 3, 64):
            _, reps = rand_replicas(9500 + R, 300, 4, R, max_e=9, max_t=4)
            _, subs = rand_replicas(9600 + R, 80, 4, R, max_e=12, max_t=6)
            rng = np.random.default_rng(9520 + R)
            pick = lambda: rng.choice(300, 80, replace=False).astype(U32)  # noqa: E731
            out["R%d-tombs-both" % R] = (reps[3], subs[0], pick(), None)   # sub: counts NULL, uniform actor
            out["R%d-tombs-rep" % R] = (reps[2], subs[1], pick(), None)    # sub: no tombs, doc_actor; rep: no doc_actor
            out["R%d-tombs-none" % R] = (_with_counts(reps[1]), subs[1], pick(), None)
            out["R%d-stale" % R] = (reps[3], subs[3], pick(), None)        # stale slack and doc_actor on both
        # --- index handling
        out["dup-low-placed"] = _simple(6, 3, 2, [(1, 0), (9, 0), (1, 1)], [4, 4, 2])
        out["dup-low-spilled"] = _simple(6, 3, 2, [(9, 0), (1, 0), (1, 1)], [4, 4, 2])
        out["oob-first"] = _simple(6, 3, 2, [(1, 0), (2, 1), (4, 0)], [6, 1, 2])
        out["oob-middle"] = _simple(6, 3, 2, [(1, 0), (2, 1), (4, 0)], [0, ONES32, 2])
        out["oob-last"] = _simple(6, 3, 2, [(1, 0), (2, 1), (4, 0)], [0, 1, 99])
        r, s, i, _ = out["R3-stale"]
        for k in (0, 1, 80, 83):
            out["n_idx-%d" % k] = (r, s, i, k)
        rep, sub, idx, _ = _simple(6, 3, 2, [(3, 2), (2, 2), (4, 1)], [5, 0, 3])
        sc, tc = sub.state.counts.copy(), sub.tombs.counts.copy()
        sc[0] += 9   # 12 live in 3 slots: clamped to 3, placed
        tc[1] += 1   # 3 live tombstones in 2 slots: clamped to 2, placed
        st = sub.state
        out["sub-count-above-slots"] = (rep, Replica(AWSetBatch(3, st.offsets, st.keys, st.actors, st.counters, st.vv, counts=sc),
                                                     TombBatch(sub.tombs.offsets, sub.tombs.keys, sub.tombs.actors,
                                                               sub.tombs.counters, counts=tc), 1, sub.doc_actor), idx, None)
        # --- gather edges: the four parities of (source, destination) come from the leads and the varying slots
        for ls in (0, 1):
            for lr in (0, 1):
                out["gather-lead%d%d" % (ls, lr)] = _gather_case(ls, lr)
        # --- spill-scan edges
        for m in (K_SCAN - 1, K_SCAN, K_SCAN + 1):
            for spill in ("none", "one", "all", "alternate"):
                out["scan-%d-%s" % (m, spill)] = _scan_case(m, spill)
        return out
    return _once("cases", make)


def big_case(n=K_PART * K_SCAN + 1):
    """n sub documents of 0 or 1 entries and tombstones onto n target documents of 0 or
    1 entry slots and 2 tombstone slots, in descending order: at the default n the spill
    scan has 1,025 partial sums, so the partials kernel takes a second step."""
    def make():
        sub = tiny_replicas(9311, n, 1, R=1, hi=2)[0]
        cap = (np.arange(n) % 3 != 0).astype(np.int64)
        off = np.zeros(n + 1, U32)
        np.cumsum(cap, out=off[1:])
        tot = int(off[-1])
        toff = (np.arange(n + 1, dtype=np.int64) * 2).astype(U32)
        rep = Replica(AWSetBatch(1, off, np.arange(tot, dtype=U64) + U64(1), np.zeros(tot, U32), np.ones(tot, U64),
                                 np.arange(n, dtype=U64), counts=cap.astype(U32)),
                      TombBatch(toff, np.arange(2 * n, dtype=U64), np.zeros(2 * n, U32), np.ones(2 * n, U64),
                                counts=np.ones(n, U32)), 0, np.zeros(n, U32))
        return rep, sub, np.arange(n - 1, -1, -1).astype(U32), None
    return _once(("big", n), make)


def history_cases(seed=9700, rounds=4):
    """rand_replicas histories: a target that receives one random sub after another,
    each result the next target (model only)."""
    _, reps = rand_replicas(seed, 200, 4, 3, max_e=9, max_t=4)
    rng = random.Random(seed)
    out = []
    for k in range(rounds):
        _, subs = rand_replicas(seed + 10 + k, 60, 4, 3, max_e=12, max_t=6)
        out.append((subs[(2, 3, 0, 2)[k]], np.array(rng.sample(range(200), 60), U32)))
    return reps[3], out
