"""The case table of the alignment-selected kernel arms, shared by
tests/test_align_cases_model.py (CPU) and tests/test_gpu_align_edges.py (GPU).

Five device calls choose between a vector arm (16 B loads and stores of keys
and counters, 8 B of actors) and a scalar arm from the alignment of the
caller's column pointers, on the host: compare and select (csrc/compare.hip),
scatter (csrc/scatter.hip), digest (csrc/digest.hip) and the worklist digest
(csrc/digest_idx.hip).  include/crdtgpu.h promises no alignment beyond the
element type, so a column that starts one element past a 16 B (8 B) boundary is
a valid argument and lands on the scalar arm.  This file holds

  shifted()          such a column, inside a pattern-filled allocation whose
                     element before and GUARD elements after the view are
                     checked afterwards,
  state_batch() ...  one deterministic state (no RNG) in two layouts, its
                     tombstones, a sub-batch and the lists every call runs on,
  compare_case()     the other side of a compare: single placed changes, the
                     flag each causes written beside it,
  pair_census()      the kernels' pair rule restated, so that the inputs are
                     known to reach the 16 B path and the element path of the
                     vector arm too,
  SHIFTS, selector() per call, the column sets to shift and the selector value
                     the launch function derives from each.
"""

import collections
import itertools

import numpy as np

from crdtgpu.batch import AWSetBatch, TombBatch
from digest_idx_cases import K_WAVE

U8, U32, U64 = np.uint8, np.uint32, np.uint64
M64 = 2 ** 64 - 1
P32, P64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A  # no key, actor, counter, clock or digest word of the table
GUARD = 64
K_CHUNK = 2048  # kCmpChunk, kSelChunk, kSctGatherChunk
R = 3
KEYS, DOTS = 1, 2  # CRDT_CMP_KEYS, CRDT_CMP_DOTS
COLUMNS = ("keys", "actors", "counters")
LAYOUTS = (0, 1)  # slack slots per document; slack 1: counts given, documents start at odd and at even slots


# ------------------------------------------------------------------ shifted columns

Shifted = collections.namedtuple("Shifted", "view big n")


def shifted(torch, t, guard=GUARD):
    """t's values in a view that starts one element past an aligned address: 8 B off 16 B
    for keys, counters and digest words, 4 B off 8 B for actors.  The allocation around it
    (one element before, `guard` after) holds the pattern; guards_intact() checks it."""
    n, size = t.numel(), t.element_size()
    big = torch.full((n + 1 + guard,), {8: P64, 4: P32}[size], dtype=t.dtype, device=t.device)
    view = big[1:1 + n]
    view.copy_(t)
    assert big.data_ptr() % (2 * size) == 0 and view.data_ptr() % (2 * size) == size
    return Shifted(view, big, n)


def guards_intact(s):
    """The element before the view and every element after it still hold the pattern."""
    h = s.big.cpu().numpy()
    pat = {8: P64, 4: P32}[h.dtype.itemsize]
    return bool(h[0] == pat and (h[1 + s.n:] == pat).all() and len(h) - 1 - s.n >= 1)


# ------------------------------------------------------------------ the state

SIZES = (0, 1, 2, 3, 63, 64, 65)
N_SMALL = 8 * len(SIZES)
FILLER, BIG = N_SMALL, N_SMALL + 1
N_DOCS = N_SMALL + 2 + 2 * len(SIZES)

_made = {}


def _once(key, make):
    if key not in _made:
        _made[key] = make()
    return _made[key]


def doc_sizes(slack):
    """Live entries per document: eight rotations of SIZES, a filler that puts the next
    document on the last slot of a 2,048-position chunk in this layout, that document
    (2,050 entries: three chunks), then two more rotations."""
    small = [SIZES[(i + r) % len(SIZES)] for r in range(8) for i in range(len(SIZES))]
    filler = (K_CHUNK - 1 - (sum(small) + len(small) * slack) - slack) % K_CHUNK
    tail = [SIZES[(i + 3) % len(SIZES)] for i in range(len(SIZES))] * 2
    return small + [filler, K_CHUNK + 2] + tail


def tomb_sizes(sizes):
    """Tombstones per document, rotated against the entries; one document whose entries
    plus tombstones are exactly the worklist digest's wave bound and one that is one above
    it (the block kernel's, like the 2,050-entry document)."""
    t = [SIZES[(d + 4) % len(SIZES)] for d in range(len(sizes))]
    t[AT_WAVE] = K_WAVE - sizes[AT_WAVE]
    t[OVER_WAVE] = K_WAVE + 1 - sizes[OVER_WAVE]
    t[FILLER], t[BIG] = 1, 3
    return t


AT_WAVE = doc_sizes(0).index(65)    # (the small documents are the same in every layout)
OVER_WAVE = doc_sizes(0).index(64)


def _live(d, n, salt):
    """(keys, actors, counters) of n entries of document d.  Keys strictly ascending, 0 first
    in every third document and 2^64 - 1 last in every third; the actors of neighbours
    differ; the counters of entries 2h and 2h + 1 differ only in the high (h even) or only
    in the low (h odd) 32 bits, and every fifth h is at or above 2^63."""
    i = np.arange(n, dtype=U64)
    keys = i * U64(1 << 52) + U64(((d + 1) * 2654435761 + salt) % (1 << 40) + 1)
    if n >= 1 and d % 3 == 0:
        keys[0] = 0
    if n >= 2 and d % 3 == 1:
        keys[-1] = M64
    actors = ((i + U64(d)) % U64(R)).astype(U32)
    h = i >> U64(1)
    sel = (h + U64(d + salt % 5)) % U64(5)
    base = np.select([sel == 0, sel == 1, sel == 2, sel == 3],
                     [h + U64(1), (h + U64(1)) << U64(32), U64(1 << 63) + h, U64(1 << 63) + ((h + U64(1)) << U64(32))],
                     U64(M64) - (h << U64(1)))
    flip = np.where(h % U64(2) == 0, U64(1 << 32), U64(1))
    counters = base ^ np.where(i & U64(1), flip, U64(0))
    return keys, actors, counters


def _column(sizes, slack, side, salt):
    """(offsets, counts, keys, actors, counters): document d holds sizes[d] live entries and
    `slack` more slots of stale entries that are another side's on every side."""
    sizes = np.asarray(sizes, np.int64)
    offsets = np.zeros(len(sizes) + 1, U32)
    np.cumsum(sizes + slack, out=offsets[1:])
    total = max(int(offsets[-1]), 1)
    slot = np.arange(total, dtype=U64)
    keys = (U64(0x7700 + side) << U64(40)) | slot
    actors = ((slot + U64(side)) % U64(R)).astype(U32)
    counters = (U64(0x1100 + side) << U64(44)) | slot
    for d, n in enumerate(sizes.tolist()):
        o = int(offsets[d])
        keys[o:o + n], actors[o:o + n], counters[o:o + n] = _live(d, n, salt)
    return offsets, sizes.astype(U32), keys, actors, counters


def _clocks(n_docs, salt):
    """Words at or above 2^63, words that differ from the next document's only in the high
    32 bits and from their neighbour's only in the low ones, a zero word in every fourth."""
    vv = np.zeros((n_docs, R), U64)
    d = np.arange(n_docs, dtype=U64)
    vv[:, 0] = U64(1 << 63) + d + U64(salt)
    vv[:, 1] = ((d + U64(1)) << U64(32)) | U64(7)
    vv[:, 2] = np.where(d % U64(4) == 3, U64(0), ((d + U64(1)) << U64(32)) | U64(8))
    return vv.reshape(-1)


def state_batch(slack, side=0, sizes=None):
    """The state in the layout `slack`: counts NULL at slack 0, given at slack 1.  sizes: the
    live sizes of another layout (the b side of a compare shares a's documents)."""
    sizes = tuple(doc_sizes(slack) if sizes is None else sizes)

    def make():
        o, c, k, a, x = _column(sizes, slack, side, 0)
        return AWSetBatch(R, o, k, a, x, _clocks(len(sizes), 0), counts=c if slack else None)
    return _once(("state", slack, side, sizes), make)


def tomb_batch(slack):
    def make():
        o, c, k, a, x = _column(tomb_sizes(doc_sizes(slack)), slack, 2, 0x5151)
        return TombBatch(o, k, a, x, c if slack else None)
    return _once(("tombs", slack), make)


# ------------------------------------------------------------------ the compare side

KINDS = ("key", "actor", "counter")
PLACES = ("pair_first", "pair_second", "doc_first", "doc_last")
FLAG = {"key": KEYS, "actor": DOTS, "counter": DOTS}  # the flag each kind of change causes
COMPARE_LAYOUTS = ((0, 0), (1, 1), (0, 1), (1, 0))  # (a's slack, b's slack)

Change = collections.namedtuple("Change", "doc kind place entry flag")


def _entry_for(place, start, n):
    """The entry of a document of n live entries starting at slot `start` that is `place`.
    pair_first / pair_second: an inner entry at an even / odd slot of a, so that both
    elements of its pair are this document's."""
    if place == "doc_first":
        return 0 if n >= 1 else None
    if place == "doc_last":
        return n - 1 if n >= 1 else None
    parity = 0 if place == "pair_first" else 1
    for i in (1, 2):
        if i <= n - 2 and (start + i) % 2 == parity:
            return i
    return None


def compare_changes(slack_a):
    """One change per changed document, about half of the documents: every kind at every
    place once in a document that starts at an even slot of a, once in one that starts at an
    odd slot, once more wherever it fits; the three-chunk document's very last key."""
    def make():
        sizes = doc_sizes(slack_a)
        starts = state_batch(slack_a).offsets.astype(np.int64)
        used, out = {BIG}, [Change(BIG, "key", "doc_last", sizes[BIG] - 1, KEYS)]
        k = 0
        for parity in (0, 1, None):
            for kind in KINDS:
                for place in PLACES:
                    for step in range(N_DOCS):
                        d = (11 * k + step) % N_DOCS
                        e = _entry_for(place, int(starts[d]), sizes[d])
                        if d not in used and e is not None and parity in (None, int(starts[d]) % 2):
                            break
                    else:
                        raise AssertionError("no document left for %s at %s" % (kind, place))
                    used.add(d)
                    out.append(Change(d, kind, place, e, FLAG[kind]))
                    k += 1
        return sorted(out)
    return _once(("changes", slack_a), make)


def compare_case(slack_a, slack_b):
    """(a, b, changes, expected flags): b holds a's documents in its own layout, with other
    stale entries in its slack, and the placed changes."""
    def make():
        sizes = doc_sizes(slack_a)
        a = state_batch(slack_a)
        s = state_batch(slack_b, 1, sizes)
        b = AWSetBatch(R, s.offsets, s.keys.copy(), s.actors.copy(), s.counters.copy(), s.vv, counts=s.counts)
        changes = compare_changes(slack_a)
        flags = np.zeros(N_DOCS, U8)
        for n, c in enumerate(changes):
            p = int(b.offsets[c.doc]) + c.entry
            if c.kind == "key":
                b.keys[p] = b.keys[p] + U64(1) if int(b.keys[p]) < M64 else U64(M64 - 1)
            elif c.kind == "actor":
                b.actors[p] = (int(b.actors[p]) + 2) % R  # neither its own nor its neighbour's
            else:
                b.counters[p] ^= U64((1, 1 << 32, 1 << 63)[n % 3])
            flags[c.doc] = c.flag
        return a, b, changes, flags
    return _once(("compare", slack_a, slack_b), make)


# ------------------------------------------------------------------ the pair census

def pair_census(spans, total):
    """The kernels' pair rule on the CPU.  spans: per document, in a's slot order,
    (its first slot in a, the index of its first entry on the partner side, live entries
    read); total: a's slot positions.  A lane takes the positions (p, p + 1) at an even p;
    with vec == 1 it reads them with 16 B loads when both are live entries of the same
    document and the partner index of the first is even, element by element otherwise.
    Returns (pairs on the 16 B path, pairs with a live position that go element by
    element, per position: 0 not read, 1 on the 16 B path, 2 element by element)."""
    doc = np.full(total + 1, -1, np.int64)
    q = np.zeros(total + 1, np.int64)
    for d, (ao, bo, n) in enumerate(spans):
        doc[ao:ao + n] = d
        q[ao:ao + n] = bo + np.arange(n)
    kind = np.zeros(total, U8)
    n_vec = n_elem = 0
    for p in range(0, total, 2):
        l0, l1 = doc[p] >= 0, doc[p + 1] >= 0
        if l0 and l1 and doc[p] == doc[p + 1] and q[p] % 2 == 0:
            kind[p] = kind[p + 1] = 1
            n_vec += 1
        elif l0 or l1:
            if l0:
                kind[p] = 2
            if l1:  # (doc[total] is no document: p + 1 < total)
                kind[p + 1] = 2
            n_elem += 1
    return n_vec, n_elem, kind


def _live_count(b, d):
    slots = int(b.offsets[d + 1]) - int(b.offsets[d])
    return slots if b.counts is None else min(int(b.counts[d]), slots)


def compare_spans(a, b):
    """compare: a's slots against b's; nothing of a document whose counts differ is read."""
    out = []
    for d in range(a.n_docs):
        na, nb = _live_count(a, d), _live_count(b, d)
        out.append((int(a.offsets[d]), int(b.offsets[d]), na if na == nb else 0))
    return out, int(a.offsets[-1])


def gather_spans(out, sources):
    """select / scatter: the packed output's positions against the source index of each
    document; sources: per output document, the first slot of the document it copies."""
    return ([(int(out.offsets[j]), int(sources[j]), int(out.counts[j])) for j in range(out.n_docs)],
            int(out.offsets[-1]))


def digest_spans(b):
    """digest: a pair is read with 16 B loads when both positions are live, whatever their
    documents; restated as the compare rule of the batch against itself."""
    return [(int(b.offsets[d]), int(b.offsets[d]), _live_count(b, d)) for d in range(b.n_docs)], int(b.offsets[-1])


# ------------------------------------------------------------------ lists and the sub-batch

def select_idx(kind):
    """identity: None.  permuted: every document once in another order (7 is coprime to
    N_DOCS), then repeats, the three-chunk document among them."""
    if kind == "identity":
        return None
    assert N_DOCS % 7 != 0
    return np.array([(7 * j + 3) % N_DOCS for j in range(N_DOCS)] + [BIG, 5, 5, AT_WAVE, BIG], U32)


SUB_DOCS = tuple(range(1, N_SMALL, 3)) + (BIG,)  # the state documents a scatter replaces, BIG among them


def sub_batch(slack):
    """Replacements of SUB_DOCS, longer, shorter and empty; the three-chunk document's is one
    entry shorter.  The list names them in descending order."""
    def make():
        sizes = [K_CHUNK + 1] + [SIZES[(j + 2) % len(SIZES)] for j in range(len(SUB_DOCS) - 1)]  # (BIG is named first)
        o, c, k, a, x = _column(sizes, slack, 3, 0xABCD)
        return AWSetBatch(R, o, k, a, x, _clocks(len(sizes), 0x99), counts=c if slack else None)
    return _once(("sub", slack), make)


def scatter_idx():
    return np.array(SUB_DOCS[::-1], U32)


def digest_list():
    """The worklist: the documents in descending order without every fifth, the documents
    on either side of the wave / block edge and the three-chunk document among them."""
    keep = [d for d in range(N_DOCS - 1, -1, -1) if d % 5 != 2 or d in (AT_WAVE, OVER_WAVE, BIG)]
    return np.array(keep, U32)


# ------------------------------------------------------------------ selectors

def cols(*batches):
    return frozenset("%s.%s" % (b, c) for b in batches for c in COLUMNS)


def _vec(shift, *batches):
    return int(not (shift & cols(*batches)))


# per call: the selector bits the launch function derives, and the shift sets that are run
BITS = {"compare": 1, "select": 1, "scatter": 2, "digest": 2, "digest_idx": 3}
SHIFTS = {
    "compare": [frozenset(), cols("a"), cols("b"), cols("a", "b")]
               + [frozenset(["%s.%s" % (s, c)]) for s in ("a", "b") for c in COLUMNS],
    "select": [frozenset(), cols("state"), cols("out"), cols("state", "out")],
    "scatter": [frozenset(), cols("state"), cols("sub"), cols("out"), cols("state", "out"), cols("sub", "out")],
    "digest": [frozenset(), cols("state"), cols("tombs"), cols("state", "tombs")],
    "digest_idx": [frozenset().union(*x) for n in range(4)
                   for x in itertools.combinations([cols("state"), cols("tombs"), frozenset(["digest"])], n)],
}
DIGEST_NULL_TOMBS = cols("state")  # run once more with tombstones NULL


def selector(call, shift):
    """The selector value of launch_<call> for columns shifted off their alignment."""
    if call == "compare":    # one conjunction of six
        return (_vec(shift, "a", "b"),)
    if call == "select":     # state and output columns
        return (_vec(shift, "state", "out"),)
    if call == "scatter":    # bit 0 vin: state and sub; bit 1 vout: the output
        return (_vec(shift, "state", "sub"), _vec(shift, "out"))
    if call == "digest":     # view_vec(st), view_vec(tb)
        return (_vec(shift, "state"), _vec(shift, "tombs"))
    if call == "digest_idx":  # vec_st, vec_tb, vec_out
        return (_vec(shift, "state"), _vec(shift, "tombs"), int("digest" not in shift))
    raise KeyError(call)


def shift_id(shift):
    if not shift:
        return "aligned"
    names = sorted(shift)
    whole = sorted({n.split(".")[0] for n in names if cols(n.split(".")[0]) <= shift or n == "digest"})
    rest = [n for n in names if n.split(".")[0] not in whole]
    return "+".join(whole + rest)
