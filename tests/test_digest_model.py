"""CPU: the per-document state digest (include/crdtgpu.h, "state digests").

digest_ref is a plain-Python restatement of the definition and the expectation
of the GPU call (tests/test_gpu_digest.py).  Here it is pinned to the known
answers of the definition, crdt_awset_digest_host is pinned to it, and both are
checked against the convergence check's restatement (compare_ref,
tests/test_compare_model.py): word 0 is equal exactly when the element sets are,
both words exactly when the live state and the clock are bit-identical.
"""

import itertools
import random

import numpy as np
import pytest

import crdtgpu
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch, TombBatch
from helpers import batch_of, ents, intern, pad, random_history, random_state
from test_compare_model import KEYS, compare_ref, golden_pairs

U32, U64 = np.uint32, np.uint64
M64 = 2 ** 64 - 1
K_E, K_T, K_A = 0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0xD6E8FEB86659FD93
K_V, K_N = 0x165667B19E3779F9, 0x85EBCA77C2B2AE63


def fmix(x):
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def doc_digest(entries, vv, deleted=()):
    """(word 0, word 1) of one document: entries / deleted [(key, actor, counter)], any order."""
    w0 = w1 = 0
    for k, a, c in entries:
        hk = fmix((k + K_E) & M64)
        w0 += hk
        w1 += fmix(hk ^ ((c + K_A * (a + 1)) & M64))
    for k, a, c in deleted:
        w1 += fmix(fmix((k + K_T) & M64) ^ ((c + K_A * (a + 1)) & M64))
    for r, v in enumerate(vv):
        if v:
            w1 += fmix((v + K_V * (r + 1)) & M64)
    n, m = len(entries), len(deleted)
    return fmix((w0 + K_N * n) & M64), fmix((w1 + K_N * (n + m)) & M64)


def _live(b, d):
    """Live (key, actor, counter) of doc d of an AWSetBatch or TombBatch, the count clamped to the slots."""
    o, e = int(b.offsets[d]), int(b.offsets[d + 1])
    slots = max(e - o, 0)
    n = min(int(b.counts[d]), slots) if b.counts is not None else slots
    return list(zip(np.asarray(b.keys[o:o + n]).tolist(), np.asarray(b.actors[o:o + n]).tolist(),
                    np.asarray(b.counters[o:o + n]).tolist()))


def digest_ref(batch, tombs=None):
    """numpy u64 [n_docs, 2]: the digest of every document of a host batch."""
    R = batch.R
    out = np.zeros((batch.n_docs, 2), U64)
    for d in range(batch.n_docs):
        vv = [int(x) for x in batch.vv[d * R:(d + 1) * R]]
        out[d] = doc_digest(_live(batch, d), vv, _live(tombs, d) if tombs is not None else ())
    return out


# (entries, vv, Deleted) -> (word 0, word 1): the known answers of the definition
KNOWN = [
    ([], [0, 0], [], (0x0000000000000000, 0x0000000000000000)),
    ([(1, 0, 1)], [1], [], (0xFE2975B1C2ADE838, 0x1442C36865B88BDD)),
    ([], [0, 2], [(7, 1, 2)], (0x0000000000000000, 0xA11B700EC9A5A949)),
    ([(1, 0, 1), (2, 1, 3), (M64, 63, 2 ** 63 + 5)], [1, 3, 0, 0], [(7, 1, 2)],
     (0x31C6D7319F301A98, 0x58C2B894EC81AD0D)),
    ([], [0, 0, 2 ** 63], [], (0x0000000000000000, 0x76D5326D0CB2DD8E)),
]


def known_batches():
    """[(AWSetBatch of one document, TombBatch or None, expected [1, 2] u64)] for KNOWN."""
    out = []
    for entries, vv, deleted, want in KNOWN:
        b = batch_of(len(vv), [(entries, vv)])
        t = TombBatch.from_lists([deleted]) if deleted else None
        out.append((b, t, np.array([want], U64)))
    return out


def with_slack(b, slack, rng):
    """The same live state with `slack` more slots per document, the slack (and a
    TombBatch's too) filled with garbage; counts given."""
    n = b.n_docs
    counts = np.array([len(_live(b, d)) for d in range(n)], U32)
    offsets = np.zeros(n + 1, U32)
    np.cumsum(counts + U32(slack), out=offsets[1:])
    total = max(int(offsets[-1]), 1)
    keys = np.array([rng.getrandbits(64) for _ in range(total)], U64)
    actors = np.array([rng.getrandbits(32) for _ in range(total)], U32)
    counters = np.array([rng.getrandbits(64) for _ in range(total)], U64)
    for d in range(n):
        for i, (k, a, c) in enumerate(_live(b, d)):
            keys[offsets[d] + i], actors[offsets[d] + i], counters[offsets[d] + i] = k, a, c
    if isinstance(b, TombBatch):
        return TombBatch(offsets, keys, actors, counters, counts)
    return AWSetBatch(b.R, offsets, keys, actors, counters, b.vv.copy(), counts=counts)


def shuffled(b, rng):
    """The same batch with every document's live entries in a random order."""
    keys, actors, counters = b.keys.copy(), b.actors.copy(), b.counters.copy()
    for d in range(b.n_docs):
        live = _live(b, d)
        rng.shuffle(live)
        o = int(b.offsets[d])
        for i, (k, a, c) in enumerate(live):
            keys[o + i], actors[o + i], counters[o + i] = k, a, c
    if isinstance(b, TombBatch):
        return TombBatch(b.offsets, keys, actors, counters, b.counts)
    return AWSetBatch(b.R, b.offsets, keys, actors, counters, b.vv, counts=b.counts)


def repadded(b, R2):
    """The same batch with every clock zero-padded to R2 >= R words."""
    vv = np.zeros(max(b.n_docs * R2, 1), U64)
    for d in range(b.n_docs):
        vv[d * R2:d * R2 + b.R] = b.vv[d * b.R:(d + 1) * b.R]
    return AWSetBatch(R2, b.offsets, b.keys, b.actors, b.counters, vv[: b.n_docs * R2], counts=b.counts)


def random_docs(seed, n_docs=60):
    """(R, AWSetBatch, TombBatch): arbitrary states (helpers.random_state) and the
    replicas of random delta histories, with their Deleted maps."""
    rng = random.Random(seed)
    R = rng.choice([1, 2, 3, 5])
    docs, tombs = [], []
    for _ in range(n_docs):
        e, vv = random_state(rng, R, rng.randint(0, 20), 64, 2 ** 40)
        docs.append((e, vv))
        tombs.append(sorted((k, rng.randrange(R), rng.randint(1, 99)) for k in rng.sample(range(64), rng.randint(0, 4))))
    reps = random_history(rng, R, 60, 12, delta=True)
    ids = intern(reps)
    for s in reps:
        docs.append((ents(s.Entries, ids), pad(s.VersionVector, R)))
        tombs.append(ents(s.Deleted, ids))
    return R, batch_of(R, docs), TombBatch.from_lists(tombs)


def test_known_answers():
    for (b, t, want), (entries, vv, deleted, w) in zip(known_batches(), KNOWN):
        assert doc_digest(entries, vv, deleted) == w
        assert (digest_ref(b, t) == want).all()
        assert (crdtgpu.digest_host(b, t) == want).all()


def test_host_equals_ref_on_random_batches():
    for seed in range(12):
        rng = random.Random(9100 + seed)
        R, b, t = random_docs(9000 + seed)
        want = digest_ref(b, t)
        assert (crdtgpu.digest_host(b, t) == want).all(), seed
        # counts and slack, the slack holding garbage
        bs, ts = with_slack(b, 1 + seed % 3, rng), with_slack(t, 2, rng)
        assert (digest_ref(bs, ts) == want).all() and (crdtgpu.digest_host(bs, ts) == want).all(), seed
        # entries in any order within a document
        assert (crdtgpu.digest_host(shuffled(bs, rng), shuffled(ts, rng)) == want).all(), seed
        assert (crdtgpu.digest_host(shuffled(b, rng), t) == want).all(), seed
        # the R padding does not show
        for R2 in (R + 1, 2 * R + 3, 64):
            assert (crdtgpu.digest_host(repadded(b, R2), t) == want).all(), (seed, R2)
            assert (digest_ref(repadded(b, R2), t) == want).all(), (seed, R2)
        # no tombstones: NULL and empty agree
        empty = TombBatch.from_lists([[] for _ in range(b.n_docs)])
        none = crdtgpu.digest_host(b)
        assert (none == digest_ref(b)).all() and (crdtgpu.digest_host(b, empty) == none).all(), seed
        assert (none[:, 0] == want[:, 0]).all()  # tombstones never reach word 0


def test_padding_tombstone_gc_and_empty_properties():
    a = crdtgpu.digest_host(batch_of(2, [([(3, 0, 5)], [5, 0])]))
    b = crdtgpu.digest_host(batch_of(4, [([(3, 0, 5)], [5, 0, 0, 0])]))
    assert (a == b).all()
    # a clock word moved to another actor does show
    assert (crdtgpu.digest_host(batch_of(2, [([(3, 0, 5)], [0, 5])])) != a).any()
    # tombstones garbage-collected on one side: word 1 differs, word 0 agrees
    st = batch_of(2, [([(3, 0, 5)], [5, 2])])
    kept = crdtgpu.digest_host(st, TombBatch.from_lists([[(9, 1, 2)]]))
    gone = crdtgpu.digest_host(st, TombBatch.from_lists([[]]))
    assert kept[0, 0] == gone[0, 0] and kept[0, 1] != gone[0, 1]
    # an entry and a tombstone of the same key and dot are told apart
    e = crdtgpu.digest_host(batch_of(1, [([(9, 0, 1)], [1])]))
    t = crdtgpu.digest_host(batch_of(1, [([], [1])]), TombBatch.from_lists([[(9, 0, 1)]]))
    assert e[0, 1] != t[0, 1]
    assert (crdtgpu.digest_host(batch_of(3, [([], [0, 0, 0])] * 4)) == 0).all()
    assert crdtgpu.digest_host(batch_of(2, [])).shape == (0, 2)


def _assert_consistent(a, b, what):
    """The digests of two batches tell exactly what compare_ref tells."""
    flags, _, _ = compare_ref(a, b)
    da, db = digest_ref(a), digest_ref(b)
    assert ((da[:, 0] != db[:, 0]) == ((flags & KEYS) != 0)).all(), what
    assert ((da != db).any(axis=1) == (flags != 0)).all(), what
    return int((flags == 0).sum()), int(((flags != 0) & ((flags & KEYS) == 0)).sum())


def test_consistent_with_compare_ref_on_every_golden_pair():
    n = n_same = n_state = 0
    for R, docs, snaps in golden_pairs():
        pairs = list(itertools.product(range(len(snaps)), repeat=2))
        a = batch_of(R, [docs[i] for i, _ in pairs])
        b = batch_of(R, [docs[j] for _, j in pairs])
        same, state = _assert_consistent(a, b, "golden")
        assert (crdtgpu.digest_host(a) == digest_ref(a)).all()
        n, n_same, n_state = n + len(pairs), n_same + same, n_state + state
    assert n >= 23 * 23 and n_same > 0 and n_state > 0


def test_consistent_with_compare_ref_on_random_pairs():
    n_same = n_state = n_keys = 0
    for seed in range(30):
        rng = random.Random(9200 + seed)
        R = rng.choice([2, 3, 5])
        reps = random_history(rng, R, rng.randint(5, 80), rng.randint(3, 20), delta=False)
        ids = intern(reps)
        docs = [(ents(s.Entries, ids), pad(s.VersionVector, R)) for s in reps]
        for x, y in itertools.permutations(reps, 2):  # and the merged states: many equal element sets
            p = x.Clone()
            p.Merge(y)
            docs.append((ents(p.Entries, ids), pad(p.VersionVector, R)))
        pairs = list(itertools.product(range(len(docs)), repeat=2))
        a = batch_of(R, [docs[i] for i, _ in pairs])
        b = batch_of(R, [docs[j] for _, j in pairs], slack=seed % 2)
        same, state = _assert_consistent(a, b, seed)
        n_same, n_state, n_keys = n_same + same, n_state + state, n_keys + len(pairs) - same - state
    assert n_same > 100 and n_state > 100 and n_keys > 100


def test_host_validation():
    u32, u64 = np.uint32, np.uint64
    lib = abi.lib()
    good = batch_of(2, [([(1, 0, 1), (4, 1, 2)], [1, 2]), ([], [0, 0])])
    out = np.zeros(4, u64)

    def rc(b, t=None, o=out):
        import ctypes

        cb = b.c() if b is not None else None
        ct = t.c() if t is not None else None
        return lib.crdt_awset_digest_host(ctypes.byref(cb) if cb else None, ctypes.byref(ct) if ct else None,
                                          o.ctypes.data if o is not None else None)

    assert rc(good) == 0
    assert rc(None) == crdtgpu.CRDT_E_INVALID and rc(good, o=None) == crdtgpu.CRDT_E_INVALID
    for R in (0, 65):
        wide = AWSetBatch(R, good.offsets, good.keys, good.actors, good.counters, np.zeros(130, u64))
        assert rc(wide) == crdtgpu.CRDT_E_INVALID
    over = batch_of(2, [([(1, 0, 1)], [1, 0])], slack=1)
    over.counts[0] = 5
    assert rc(over) == crdtgpu.CRDT_E_CAPACITY
    back = AWSetBatch(2, np.array([0, 2, 1], u32), good.keys, good.actors, good.counters, good.vv)
    assert rc(back) == crdtgpu.CRDT_E_INVALID
    nokeys = AWSetBatch(2, good.offsets, None, good.actors, good.counters, good.vv)
    assert rc(nokeys) == crdtgpu.CRDT_E_INVALID
    n = 3
    tb = lambda offs, counts=None: TombBatch(np.array(offs, u32), np.arange(n).astype(u64), np.zeros(n, u32),  # noqa: E731
                                             np.ones(n, u64), None if counts is None else np.array(counts, u32))
    assert rc(good, tb([0, 2, 3])) == 0
    assert rc(good, tb([0, 3, 2])) == crdtgpu.CRDT_E_INVALID
    assert rc(good, tb([0, 2, 3], counts=[3, 1])) == crdtgpu.CRDT_E_CAPACITY
    assert rc(good, TombBatch(None, None, None, None)) == crdtgpu.CRDT_E_INVALID
    with pytest.raises(crdtgpu.CrdtError):
        crdtgpu.digest_host(over)


def test_header_and_library_have_the_entry_points():
    names = ("crdt_awset_digest_async", "crdt_awset_digest_host", "crdt_digest_diff_async")
    have = crdtgpu.header_functions()
    for name in names:
        assert name in have and name in abi.signatures()
        assert getattr(abi.lib(), name) is not None  # exported by libcrdtgpu.so
    assert (crdtgpu.CRDT_DIG_ELEMENTS, crdtgpu.CRDT_DIG_STATE) == (crdtgpu.CRDT_CMP_KEYS, crdtgpu.CRDT_CMP_DOTS)
