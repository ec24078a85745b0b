"""Shared by tests/test_sources_model.py (CPU) and tests/test_gpu_sources.py:
sources_ref, the numpy restatement of crdt_awset_sources_async's contract
(include/crdtgpu.h), and the replica builders both files draw their cases from.

A replica's documents are lists docs[d] = (entries, tombstones, vv) with entries
and tombstones [(key, actor, counter)] ascending by key; make_replica packs them
into the resident layout (offsets, optional counts, slack after each live
prefix, stale values in the slack) and host_built packs the same documents with
SrcBatch.from_lists, the host builder the call replaces.
"""

import numpy as np

from crdtgpu.batch import AWSetBatch, Replica, SrcBatch, TombBatch

U32, U64 = np.uint32, np.uint64
ONES32 = 2 ** 32 - 1
MAXK = 2 ** 64 - 1
K_SCAN = 1024     # kSrcScanChunk: sources per workgroup of the offset scan
K_PART = 1024     # kSrcPartStep: partial sums per step of the partials scan
K_GATHER = 2048   # kSrcGatherChunk: output positions per gather step
K_RUN = 1024      # kSrcRun: sources of a gather chunk staged in LDS at most


# ------------------------------------------------------------------ reference

class SourcesRef:
    """msg: the whole packed source batch (arrays as long as the totals); n_e /
    n_t: entries / tombstones the call writes (the totals, cut at the slot
    limits); capacity: crdt_ctx_sync reports CRDT_E_CAPACITY."""

    def __init__(self, msg, n_e, n_t, capacity):
        self.msg, self.n_e, self.n_t, self.capacity = msg, n_e, n_t, capacity


def _live(off, cnt):
    """(clamped live count per document as int64, some count was above its slots)."""
    o = np.asarray(off, U32).astype(np.int64)
    slots = np.maximum(o[1:] - o[:-1], 0)
    live = slots if cnt is None else np.asarray(cnt, U32).astype(np.int64)
    return np.minimum(live, slots), bool((live > slots).any())


def _pack(cols, counts, n, P):
    """cols[p]: (offsets, keys, actors, counters) or None; counts[p]: int64 [n].
    -> (u32 offsets [n*P+1], keys, actors, counters, 64-bit total), source-major."""
    c = np.stack(counts, axis=1).reshape(-1) if n else np.zeros(0, np.int64)
    off = np.zeros(n * P + 1, np.int64)
    np.cumsum(c, out=off[1:])
    total = int(off[-1])
    keys, actors, counters = np.zeros(total, U64), np.zeros(total, U32), np.zeros(total, U64)
    at = off[:-1].reshape(n, P)
    for p, col in enumerate(cols):
        cp = counts[p]
        m = int(cp.sum())
        if col is None or m == 0:
            continue
        ramp = np.arange(m, dtype=np.int64) - np.repeat(np.cumsum(cp) - cp, cp)
        src = np.repeat(np.asarray(col[0], U32)[:-1].astype(np.int64), cp) + ramp
        dst = np.repeat(at[:, p], cp) + ramp
        keys[dst], actors[dst], counters[dst] = (np.asarray(col[1], U64)[src], np.asarray(col[2], U32)[src],
                                                 np.asarray(col[3], U64)[src])
    return (off % (1 << 32)).astype(U32), keys, actors, counters, total


def sources_ref(replicas, entry_slots=None, tomb_slots=None):
    """What crdt_awset_sources_async writes for host replicas (crdtgpu.batch.Replica
    over numpy arrays), vectorised over documents."""
    P = len(replicas)
    st0 = replicas[0].state
    n, R = st0.n_docs, st0.R
    assert 1 <= P <= 16 and all(r.state.n_docs == n and r.state.R == R for r in replicas)
    over = False
    ce, ct, ecols, tcols = [], [], [], []
    for r in replicas:
        s, t = r.state, r.tombs
        c, o = _live(s.offsets, s.counts)
        over |= o
        ce.append(c)
        ecols.append((s.offsets, s.keys, s.actors, s.counters))
        if t is None:
            ct.append(np.zeros(n, np.int64))
            tcols.append(None)
        else:
            c, o = _live(t.offsets, t.counts)
            over |= o
            ct.append(c)
            tcols.append((t.offsets, t.keys, t.actors, t.counters))
    eoff, k, a, c, te = _pack(ecols, ce, n, P)
    toff, tk, ta, tc, tt = _pack(tcols, ct, n, P)
    actor = np.stack([np.asarray(r.doc_actor, U32) if r.doc_actor is not None else np.full(n, r.actor, U32)
                      for r in replicas], axis=1).reshape(-1)
    vv = np.stack([np.asarray(r.state.vv, U64)[: n * R].reshape(n, R) for r in replicas], axis=1).reshape(-1)
    doc_srcs = (np.arange(n + 1, dtype=np.int64) * P).astype(U32)
    msg = SrcBatch(R, doc_srcs, actor, vv, eoff, k, a, c, toff, tk, ta, tc)
    n_e = te if entry_slots is None else min(te, int(entry_slots))
    n_t = tt if tomb_slots is None else min(tt, int(tomb_slots))
    return SourcesRef(msg, n_e, n_t, over or n_e < te or n_t < tt)


def same_sources(a, b):
    """Two host source batches hold the same message (arrays may be padded past the totals)."""
    ns = a.n_srcs
    if not (a.R == b.R and a.n_docs == b.n_docs and ns == b.n_srcs):
        return False
    ok = (a.doc_srcs == b.doc_srcs).all() and (a.src_actor == b.src_actor).all()
    ok = ok and (a.vv[: ns * a.R] == b.vv[: ns * a.R]).all()
    ok = ok and (a.entry_off == b.entry_off).all() and (a.tomb_off == b.tomb_off).all()
    te, tt = int(a.entry_off[-1]), int(a.tomb_off[-1])
    for f, m in (("keys", te), ("actors", te), ("counters", te), ("tkeys", tt), ("tactors", tt), ("tcounters", tt)):
        ok = ok and (getattr(a, f)[:m] == getattr(b, f)[:m]).all()
    return bool(ok)


# ------------------------------------------------------------------- builders

def rand_list(rng, R, n, bits=40):
    """n (key, actor, counter) ascending by key; rng: random.Random."""
    ks = set()
    if n and rng.random() < 0.2:
        ks.add(0)
    if n > 1 and rng.random() < 0.2:
        ks.add(MAXK)
    while len(ks) < n:
        ks.add(rng.getrandbits(64))
    return [(k, rng.randrange(R), rng.randint(1, 2 ** bits)) for k in sorted(ks)]


def rand_docs(rng, R, n_docs, max_e=12, max_t=4):
    """Documents of 0..max_e entries and 0..max_t tombstones; every 7th is empty and
    every 11th holds only tombstones."""
    docs = []
    for d in range(n_docs):
        ne, nt = rng.randint(0, max_e), rng.randint(0, max_t)
        if d % 7 == 3:
            ne = nt = 0
        elif d % 11 == 5:
            ne, nt = 0, max(nt, 1)
        docs.append((rand_list(rng, R, ne), rand_list(rng, R, nt), [rng.randint(0, 2 ** 40) for _ in range(R)]))
    return docs


def pack_cols(lists, slack=0, with_counts=False, garbage=None, lead=0):
    """[(key, actor, counter)] per document -> (offsets, counts or None, keys, actors,
    counters): `slack` slots after each live prefix, filled from the numpy rng
    `garbage` (stale, non-zero) when given; `lead`: unused slots before the first
    document (offsets[0] = lead), which makes every source run start at another parity."""
    n = len(lists)
    counts = np.array([len(x) for x in lists], U32)
    offsets = np.zeros(n + 1, U32)
    np.cumsum(counts + U32(slack), out=offsets[1:])
    offsets += U32(lead)
    total = int(offsets[-1])
    m = max(total, 1)
    if garbage is not None:
        keys = garbage.integers(1, 2 ** 63, m, dtype=np.int64).view(U64).copy()
        actors = garbage.integers(1, 2 ** 31, m, dtype=np.int64).astype(U32)
        counters = garbage.integers(1, 2 ** 63, m, dtype=np.int64).view(U64).copy()
    else:
        keys, actors, counters = np.zeros(m, U64), np.zeros(m, U32), np.zeros(m, U64)
    flat = [e for x in lists for e in x]
    if flat:
        lens = counts.astype(np.int64)
        pos = np.repeat(offsets[:-1].astype(np.int64), lens) + (np.arange(len(flat)) - np.repeat(np.cumsum(lens) - lens, lens))
        keys[pos] = np.array([e[0] for e in flat], U64)
        actors[pos] = np.array([e[1] for e in flat], U32)
        counters[pos] = np.array([e[2] for e in flat], U64)
    return offsets, (counts if (slack or with_counts) else None), keys, actors, counters


def make_replica(R, docs, slack=0, with_counts=False, garbage=None, tombs=True, actor=0, doc_actor=None, lead=0):
    """The resident (host) form of one replica's documents."""
    n = len(docs)
    o, c, k, a, n_ = pack_cols([d[0] for d in docs], slack, with_counts, garbage, lead)
    vv = np.array([d[2] for d in docs], U64).reshape(-1) if n else np.zeros(0, U64)
    state = AWSetBatch(R, o, k, a, n_, vv, counts=c)
    tb = None
    if tombs:
        to, tc, tk, ta, tn = pack_cols([d[1] for d in docs], slack, with_counts, garbage, lead)
        tb = TombBatch(to, tk, ta, tn, counts=tc)
    return Replica(state, tb, actor=actor, doc_actor=None if doc_actor is None else np.asarray(doc_actor, U32))


def host_built(R, reps_docs, replicas):
    """SrcBatch.from_lists of each replica's live documents, in replica order
    (a replica without tombstones contributes none)."""
    n = len(reps_docs[0])
    per_doc = []
    for d in range(n):
        srcs = []
        for docs, r in zip(reps_docs, replicas):
            actor = int(r.doc_actor[d]) if r.doc_actor is not None else r.actor
            srcs.append((actor, docs[d][2], docs[d][0], docs[d][1] if r.tombs is not None else None))
        per_doc.append(srcs)
    return SrcBatch.from_lists(R, per_doc)


LAYOUTS = [dict(slack=0, with_counts=False), dict(slack=0, with_counts=True), dict(slack=3, with_counts=True),
           dict(slack=3, with_counts=True, garbage=True)]


def rand_replicas(seed, n_docs, P, R, max_e=12, max_t=4):
    """P replicas in mixed layouts: replica p takes LAYOUTS[p % 4] (slack 0 and 3,
    counts given and NULL, stale non-zero slack), replica 1 has no tombstones, odd
    replicas name their actor per document.  -> (reps_docs, replicas)."""
    import random

    rng = random.Random(seed)
    reps_docs, replicas = [], []
    for p in range(P):
        docs = rand_docs(rng, R, n_docs, max_e, max_t)
        lay = dict(LAYOUTS[p % len(LAYOUTS)])
        if lay.pop("garbage", False):
            lay["garbage"] = np.random.default_rng(seed + p)
        doc_actor = [rng.randrange(R) for _ in range(n_docs)] if p % 2 else None
        replicas.append(make_replica(R, docs, tombs=(p != 1), actor=p % R, doc_actor=doc_actor, **lay))
        reps_docs.append(docs)
    return reps_docs, replicas


def tiny_replicas(seed, n_docs, P, R=1, hi=3):
    """P replicas of n_docs documents of 0..hi-1 entries and 0..1 tombstones, built with
    numpy alone (n_docs may be large); one slack slot per document."""
    rng = np.random.default_rng(seed)
    reps = []
    for p in range(P):
        def cols(hi_):
            cnt = rng.integers(0, hi_, n_docs).astype(U32)
            off = np.zeros(n_docs + 1, U32)
            np.cumsum(cnt + U32(1), out=off[1:])
            tot = int(off[-1])
            return (off, cnt, np.arange(tot, dtype=U64) * U64(3) + U64(p),
                    rng.integers(0, R, tot, dtype=np.int64).astype(U32),
                    rng.integers(1, 2 ** 40, tot, dtype=np.int64).view(U64).copy())
        o, c, k, a, n_ = cols(hi)
        to, tc, tk, ta, tn = cols(2)
        vv = rng.integers(0, 99, n_docs * R, dtype=np.int64).view(U64).copy()
        reps.append(Replica(AWSetBatch(R, o, k, a, n_, vv, counts=c), TombBatch(to, tk, ta, tn, counts=tc), actor=p % R))
    return reps
