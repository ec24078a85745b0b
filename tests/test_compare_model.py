"""CPU: the convergence check and the sub-batch selection restated over the
packed layout.

compare_ref and select_ref are the expectations of the GPU calls
(tests/test_gpu_compare.py, crdt_awset_compare_* / crdt_awset_select_async):
plain numpy / dict restatements of the contract in include/crdtgpu.h.  Only the
live prefix of a document -- its first counts[d] slots -- is ever looked at.
compare_ref is pinned here against the reference's own notion of convergence,
assertEntries (equal sorted values), on every pair of states recorded in
tests/golden/kat_scenarios.json, and against the map restatement of the
reference (oracle/awset_ref.py): after an exchange the two replicas hold the
same elements.
"""

import itertools
import json
import random

import numpy as np

import crdtgpu
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch
from helpers import GOLDEN, batch_of, ents, intern, pad, random_history, snap_entries

U8, U32, U64 = np.uint8, np.uint32, np.uint64
KEYS, DOTS, A_AHEAD, B_AHEAD = 1, 2, 4, 8


def _live(b, d):
    """(keys, actors, counters) lists of doc d's live entries, the count clamped to the slots."""
    o, e = int(b.offsets[d]), int(b.offsets[d + 1])
    slots = max(e - o, 0)
    n = min(int(b.counts[d]), slots) if b.counts is not None else slots
    return (np.asarray(b.keys[o:o + n]).tolist(), np.asarray(b.actors[o:o + n]).tolist(),
            np.asarray(b.counters[o:o + n]).tolist())


def compare_ref(a, b, mask=15):
    """(flags u8 [n_docs], summary u32 [5], worklist u32 [n_work]) of two host batches."""
    assert a.n_docs == b.n_docs and a.R == b.R
    n, R = a.n_docs, a.R
    flags = np.zeros(n, U8)
    for d in range(n):
        ka, aa, ca = _live(a, d)
        kb, ab, cb = _live(b, d)
        f = 0
        if ka != kb:
            f |= KEYS
        elif aa != ab or ca != cb:
            f |= DOTS
        va = [int(x) for x in a.vv[d * R:(d + 1) * R]]
        vb = [int(x) for x in b.vv[d * R:(d + 1) * R]]
        if any(x > y for x, y in zip(va, vb)):
            f |= A_AHEAD
        if any(y > x for x, y in zip(va, vb)):
            f |= B_AHEAD
        flags[d] = f
    work = np.nonzero(flags & U8(mask))[0].astype(U32)
    summary = np.array([int(((flags >> k) & 1).sum()) for k in range(4)] + [len(work)], U32)
    return flags, summary, work


def select_ref(state, idx=None, n_idx=None, n_out=None):
    """The packed batch select writes: doc j = state doc idx[j] for j < n_idx,
    empty (count 0, VV zeros) beyond; an idx[j] that is no document: empty too."""
    n_out = state.n_docs if n_out is None else int(n_out)
    n_idx = n_out if n_idx is None else min(int(n_idx), n_out)
    R = state.R
    docs = []
    for j in range(n_out):
        d = (int(idx[j]) if idx is not None else j) if j < n_idx else None
        if d is None or d >= state.n_docs:
            docs.append(([], [0] * R))
        else:
            k, a, c = _live(state, d)
            docs.append((list(zip(k, a, c)), [int(x) for x in state.vv[d * R:(d + 1) * R]]))
    counts = np.array([len(e) for e, _ in docs], U32)
    offsets = np.zeros(n_out + 1, U32)
    np.cumsum(counts, out=offsets[1:])
    total = int(offsets[-1])
    keys, actors, counters = np.zeros(total, U64), np.zeros(total, U32), np.zeros(total, U64)
    vv = np.zeros(n_out * R, U64)
    for j, (e, v) in enumerate(docs):
        o = int(offsets[j])
        if e:
            keys[o:o + len(e)] = [x[0] for x in e]
            actors[o:o + len(e)] = [x[1] for x in e]
            counters[o:o + len(e)] = [x[2] for x in e]
        vv[j * R:(j + 1) * R] = v
    return AWSetBatch(R, offsets, keys, actors, counters, vv, counts=counts)


def golden_pairs():
    """Per scenario: (R, the snapshots as packed docs, the snapshots) -- every
    state the fixture records, over one key universe per scenario."""
    g = json.load(open(GOLDEN))
    out = []
    for sc in g["scenarios"]:
        snaps = list(sc["final"].values())
        for m in sc["merges"]:
            snaps += [m["dst"], m["src"], m["out"]]
        universe = sorted({e[0] for s in snaps for e in s["entries"] + s.get("deleted", [])})
        ids = {k: i for i, k in enumerate(universe)}
        R = max(len(s["vv"]) for s in snaps)
        docs = [(snap_entries(s, ids), pad(s["vv"], R)) for s in snaps]
        out.append((R, docs, snaps))
    return out


def test_compare_ref_is_assert_entries_on_every_golden_pair():
    n_pairs = n_equal = 0
    for R, docs, snaps in golden_pairs():
        pairs = list(itertools.product(range(len(snaps)), repeat=2))
        a = batch_of(R, [docs[i] for i, _ in pairs])
        b = batch_of(R, [docs[j] for _, j in pairs])
        flags, summary, work = compare_ref(a, b)
        for p, (i, j) in enumerate(pairs):
            same = sorted(e[0] for e in snaps[i]["entries"]) == sorted(e[0] for e in snaps[j]["entries"])  # assertEntries
            assert bool(flags[p] & KEYS) == (not same), (i, j)
            n_equal += same
        assert summary[4] == len(work) and (np.diff(work.astype(np.int64)) > 0).all()
        n_pairs += len(pairs)
    assert n_pairs >= 23 * 23 and 0 < n_equal < n_pairs


def test_exchange_directions_share_their_elements():
    """a <- b and b <- a (the reference's Merge, map restatement) hold the same
    elements: KEYS never set, whatever DOTS and the clocks say."""
    n = n_dots = 0
    for seed in range(40):
        rng = random.Random(8000 + seed)
        R = rng.choice([2, 3, 5])
        reps = random_history(rng, R, rng.randint(5, 80), rng.randint(3, 30), delta=False)
        ids = intern(reps)
        ab, ba = [], []
        for x, y in itertools.permutations(reps, 2):
            p, q = x.Clone(), y.Clone()
            p.Merge(y)
            q.Merge(x)
            ab.append((ents(p.Entries, ids), pad(p.VersionVector, R)))
            ba.append((ents(q.Entries, ids), pad(q.VersionVector, R)))
        flags, _, _ = compare_ref(batch_of(R, ab), batch_of(R, ba, slack=seed % 3))
        assert not (flags & KEYS).any(), seed
        assert not (flags & (A_AHEAD | B_AHEAD)).any(), seed  # both clocks are the elementwise max
        n += len(ab)
        n_dots += int(((flags & DOTS) != 0).sum())
    assert n > 200


def _random_batch(rng, n, R, slack=0):
    docs = []
    for _ in range(n):
        k = sorted(rng.sample(range(40), rng.randint(0, 12)))
        docs.append(([(x, rng.randrange(R), rng.randint(1, 9)) for x in k], [rng.randint(0, 9) for _ in range(R)]))
    return batch_of(R, docs, slack=slack)


def test_identities():
    rng = random.Random(8100)
    R, n = 3, 300
    x, y = _random_batch(rng, n, R), _random_batch(rng, n, R, slack=2)
    for d in range(0, n, 3):  # a third of the documents equal on both sides
        o, c = int(y.offsets[d]), int(x.offsets[d + 1]) - int(x.offsets[d])
        y.counts[d] = c if c <= int(y.offsets[d + 1]) - o else 0
        if y.counts[d] == c:
            xo = int(x.offsets[d])
            y.keys[o:o + c], y.actors[o:o + c], y.counters[o:o + c] = (
                x.keys[xo:xo + c], x.actors[xo:xo + c], x.counters[xo:xo + c])
            if d % 2 and c:  # ... and half of those under one other dot
                y.counters[o + c - 1] += 1
    flags, summary, work = compare_ref(x, x)
    assert not flags.any() and not summary.any() and len(work) == 0
    f_xy, s_xy, _ = compare_ref(x, y)
    f_yx, s_yx, _ = compare_ref(y, x)
    assert (f_xy & 3 == f_yx & 3).all()
    assert (((f_xy >> 2) & 1) == ((f_yx >> 3) & 1)).all() and (((f_xy >> 3) & 1) == ((f_yx >> 2) & 1)).all()
    assert 0 < s_xy[0] < n and s_xy[1] > 0 and (s_xy[:2] == s_yx[:2]).all() and s_xy[2] == s_yx[3]
    assert not (f_xy & KEYS)[(f_xy & DOTS) != 0].any()  # DOTS only under equal element sets
    for mask in (0, 1, 2, 4, 8, 15):
        f, s, w = compare_ref(x, y, mask)
        assert (f == f_xy).all() and w.tolist() == [d for d in range(n) if f[d] & mask] and s[4] == len(w)
    packed = select_ref(y)
    assert int(packed.offsets[-1]) == int(y.counts.sum())  # no slack
    assert not compare_ref(packed, y)[0].any()
    # a selection: order and repeats kept, the tail and an index that is no document empty
    idx = np.array([5, 2, 2, n, 0], U32)
    sel = select_ref(y, idx, n_idx=4, n_out=6)
    assert sel.n_docs == 6 and sel.doc(0) == y.doc(5) and sel.doc(1) == sel.doc(2) == y.doc(2)
    for j in (3, 4, 5):
        assert sel.doc(j) == ([], [0] * R)


def test_header_and_library_have_the_entry_points():
    names = ("crdt_awset_compare_async", "crdt_awset_compare_batch", "crdt_awset_select_async")
    have = crdtgpu.header_functions()
    for name in names:
        assert name in have and name in abi.signatures()
        assert getattr(abi.lib(), name) is not None  # exported by libcrdtgpu.so
    assert (crdtgpu.CRDT_CMP_KEYS, crdtgpu.CRDT_CMP_DOTS, crdtgpu.CRDT_CMP_A_AHEAD, crdtgpu.CRDT_CMP_B_AHEAD) == \
        (KEYS, DOTS, A_AHEAD, B_AHEAD)
