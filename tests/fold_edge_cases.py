"""Deterministic fold cases that sit on every dispatch edge of csrc/fold.hip.

Each builder returns a Case: one or more (dst, srcs) batches for one fold mode,
and the classes of tests/fold_paths.py's census the case is built to hit (the
CPU test asserts at least 8 documents in each).  Seeded; counters and clocks
stay within 1..64 so that every case can go through tests/counter_maps.py.

States are not drawn blindly: with arbitrary clocks an ordered fold of many
sources empties most documents.  Every document has a low clock ceiling H; a
dot's counter is either above it ("high": never seen by any clock, so the entry
is added, wins and survives, a tombstone deletes) or at most H ("low": covered
sooner or later, so the entry is skipped or removed, a tombstone is ignored).
Mixing the two makes adds, skips, replaced dots and removals all reach the
output (tests/test_fold_paths_model.py checks that they do, per case).
"""

from __future__ import annotations

import functools
import random
from typing import Callable, List, NamedTuple, Tuple

import numpy as np

import fold_paths as fp
from crdtgpu import CRDT_FOLD_AWSET, CRDT_FOLD_DELTA
from crdtgpu.batch import AWSetBatch, SrcBatch

AWSET, DELTA = CRDT_FOLD_AWSET, CRDT_FOLD_DELTA
MODES = (AWSET, DELTA)
U32, U64 = np.uint32, np.uint64
TOP = (1 << 64) - 1
H = 8        # clock ceiling of a document
CMAX = 64    # counters fit the tables of tests/counter_maps.py

SOURCE_RUNGS = (15, 16, 17, 31, 32, 33, 63, 64, 65, 66, 100)
LADDER_R = {AWSET: (2, 1, 3), DELTA: (4, 2)}
DOC_COUNTS = {AWSET: (1, 2, 31, 32, 33, 63, 64, 65, 449, 512, 513, 581, 1087),
              DELTA: (1, 7, 8, 9, 57, 64, 65, 75, 137)}


class Case(NamedTuple):
    name: str
    mode: int
    batches: List[Tuple[AWSetBatch, SrcBatch]]
    # (label, lean_first, predicate over a fold_paths record): >= 8 documents each
    classes: List[Tuple[str, int, Callable[[dict], bool]]]


def mode_name(mode):
    return "delta" if mode == DELTA else "awset"


# ---------------------------------------------------------------- one document

def dot(rng, R, high, actors=None):
    a = rng.choice(actors) if actors else rng.randrange(R)
    return a, (rng.randint(H + 1, CMAX) if high else rng.randint(1, H))


def entries(rng, R, keys, p_hi=0.5, actors=None):
    return [(k,) + dot(rng, R, rng.random() < p_hi, actors) for k in sorted(keys)]


def make_doc(rng, R, delta, ms, n_dst, universe, ents=(0, 2), tombs=(0, 1), feature=None, p_hi=0.5):
    """(dst entries, dst clock, chain) of one document.

    universe: the keys the document draws from (a list of ints).
    feature (delta folds): None; "first" -- one source, past position 32 when the
    chain is that long, is a first contact (its actor's counter is 0 in every
    clock before it: R - 1 is kept for it); "noop" -- one such source brings
    nothing (its one entry is covered, no tombstones) but carries a high clock
    entry, so the prefix-max clocks after it are not the exact ones, and a later
    source has an entry between the two."""
    reserve = delta and feature == "first" and R >= 2 and ms >= 1
    acts = list(range(R - 1)) if reserve else list(range(R))
    pos = (rng.randint(33, ms - 2) if ms >= 36 else rng.randint(ms // 2, ms - 1)) if ms >= 1 else 0
    vv = [rng.randint(1, H) for _ in range(R)]
    if reserve:
        vv[R - 1] = 0
    dst = entries(rng, R, rng.sample(universe, min(n_dst, len(universe))), p_hi, acts)
    dkeys = [k for k, _, _ in dst]
    chain = []
    for j in range(ms):
        svv = [rng.randint(0, H) for _ in range(R)]
        if reserve and j < pos:
            svv[R - 1] = 0
        actor = rng.choice(acts)
        if reserve and j == pos:
            actor = R - 1
        e = entries(rng, R, rng.sample(universe, min(rng.randint(*ents), len(universe))), p_hi, acts)
        t = []
        if delta:
            for _ in range(rng.randint(*tombs)):
                r = rng.random()
                if e and r < 0.45:  # a key this source also holds: re-added, or the same dot
                    k, a, c = rng.choice(e)
                    how = rng.randrange(3)
                    if how == 0:
                        t.append((k, a, c))                      # same dot: still a tombstone
                    elif how == 1 and len(acts) > 1:
                        t.append((k, rng.choice([x for x in acts if x != a]), c))  # another actor: re-added
                    else:
                        t.append((k, a, c - 1) if c > 1 else (k, a, c))  # a higher counter since: re-added
                else:
                    k = rng.choice(dkeys) if dkeys and r < 0.8 else rng.choice(universe)
                    t.append((k,) + dot(rng, R, rng.random() < 0.6, acts))
            t = sorted({k: (k, a, c) for k, a, c in t}.values())
            # no accidental no-op step: a source brings a high entry, or a tombstone it has not re-added
            held = {k for k, _, _ in e}
            if not any(c > H for _, _, c in e) and not any(k not in held for k, _, _ in t):
                k = rng.choice([x for x in universe if x not in held])
                e = sorted(e + [(k,) + dot(rng, R, True, acts)])
        if delta and feature == "noop" and j == pos:
            a = rng.choice(acts)
            e, t = [(rng.choice(universe), a, 1)], []
            svv[a] = 40
            chain.append((actor, svv, e, t))
            continue
        if delta and feature == "noop" and j == pos + 1:
            a = chain[pos][2][0][1]
            k = rng.choice(universe)
            e = sorted([x for x in e if x[0] != k] + [(k, a, 30)])
        chain.append((actor, svv, e, t))
    return dst, vv, chain


def batches_of(R, docs):
    return (AWSetBatch.from_docs(R, [(e, vv) for e, vv, _ in docs]),
            SrcBatch.from_lists(R, [c for _, _, c in docs]))


# ---------------------------------------------------------------- source ladder

@functools.lru_cache(maxsize=None)
def source_ladder(mode, R, per_rung=30):
    """ms in SOURCE_RUNGS, 0..2 entries and (delta) 0..1 tombstones a source, 0..20
    entries in dst, keys within 40 ids.  Delta folds: a third of the documents hold a
    first contact, a third a no-op step -- past position 32 on the longer chains."""
    delta = mode == DELTA
    rng = random.Random(9000 + 10 * R + mode)
    docs = []
    for ms in SOURCE_RUNGS:
        for d in range(per_rung):
            base = rng.randrange(0, 1 << 20)
            feature = (None, "first", "noop")[d % 3] if delta else None
            docs.append(make_doc(rng, R, delta, ms, rng.randint(0, 20), list(range(base, base + 40)), feature=feature))
    cl = []
    gen_cap = fp.vcap(mode, False)
    for lean in (1, 0):
        for ms in SOURCE_RUNGS[1:]:
            p = "block" if ms > fp.T("MCAP") or ms * R > gen_cap else ("general-deferred" if lean else "general-direct")
            cl.append(("ms=%d: %s lean=%d" % (ms, p, lean), lean,
                       (lambda ms, p: lambda r: r["ms"] == ms and r["pass"] == p)(ms, p)))
    cl.append(("lean ms=15", 1, lambda r: r["pass"] == "lean" and r["ms"] == 15))
    if delta:
        cl += [("binary search, both verdicts", 0, lambda r: r["tomb_search"] == "binary" and len(r["readd"]) == 2),
               ("noop replay ms>32", 0, lambda r: r["noop_replay"] and r["ms"] > 32),
               ("lean defers: full step", 1, lambda r: r["lean_why"] == "full-step" and r["ms"] == 15),
               ("lean defers: noop step", 1, lambda r: r["lean_why"] == "noop-step" and r["ms"] == 15)]
    if R * 64 > gen_cap:
        cl.append(("block: clocks at ms=64", 0, lambda r: r["why"] == "clocks" and r["ms"] == 64))
    return Case("source_ladder_%s_R%d" % (mode_name(mode), R), mode, [batches_of(R, docs)], cl)


# ---------------------------------------------------------------- tuple ladder

def sized_doc(rng, R, delta, n, E, X, ms, universe, wide_dst=False, keep_all=False):
    """A document of exactly n + E + X tuples over ms sources.  keep_all (delta): no
    full step, every entry changed, every tombstone effective -- every tuple kept."""
    assert ms > 0 or E + X == 0
    vv = [rng.randint(1, H) for _ in range(R)]
    keys = rng.sample(universe, n)
    if wide_dst and n >= 2:
        keys = sorted(keys)
        keys[0], keys[-1] = min(universe) - 1, max(universe) + 5000
    dst = entries(rng, R, keys, 1.0 if keep_all else 0.5)
    chain = []
    for j in range(ms):
        ne = E // ms + (1 if j < E % ms else 0)
        nx = X // ms + (1 if j < X % ms else 0)
        ks = rng.sample(universe, ne + nx)  # tombstones on keys the source does not hold: effective
        e = entries(rng, R, ks[:ne], 1.0 if keep_all else 0.5)
        t = entries(rng, R, ks[ne:], 1.0 if keep_all else 0.6) if delta else []
        svv = [rng.randint(0, H) for _ in range(R)]
        chain.append((rng.randrange(R), svv, e, t))
    return dst, vv, chain


@functools.lru_cache(maxsize=None)
def tuple_ladder(mode):
    """n + E + X at cap - 1, cap, cap + 1 (cap 128 AWSet / 256 delta), all in dst, all
    in the sources, and even; kept tuples at 64 / 65 and 128 / 129 on the sort path."""
    delta = mode == DELTA
    R = 3
    cap = fp.ncap(mode)
    rng = random.Random(9100 + mode)
    docs = []
    for rep in range(16):
        for N in (cap - 1, cap, cap + 1):
            uni = list(range(1000 * rep, 1000 * rep + 400))
            docs.append(sized_doc(rng, R, delta, N, 0, 0, 0 if rep % 2 else 2, uni))         # all in dst
            X = N // 4 if delta else 0
            docs.append(sized_doc(rng, R, delta, 0, N - X, X, 8, uni))                       # all in sources
            n = N // 3
            X = N // 3 if delta else 0
            docs.append(sized_doc(rng, R, delta, n, N - n - X, X, 6, uni))                   # even
        for Kc in ((64, 65, 128, 129) if delta else (64, 65)):
            uni = list(range(5000 * rep + 100000, 5000 * rep + 100300))
            n = Kc // 2
            X = Kc // 4 if delta else 0
            docs.append(sized_doc(rng, R, delta, n, Kc - n - X, X, 5, uni, wide_dst=True, keep_all=delta))
    cl = [("N = cap - 1 on the pipe", 0, lambda r: r["N"] == cap - 1 and r["pass"] == "general-direct"),
          ("N = cap on the pipe", 0, lambda r: r["N"] == cap and r["pass"] == "general-direct"),
          ("N = cap + 1 on the block path", 0, lambda r: r["N"] == cap + 1 and r["why"] == "tuples"),
          ("N = cap + 1, lean defers then block", 1, lambda r: r["N"] == cap + 1 and r["lean_why"] == "tuples"),
          ("block ms=0", 0, lambda r: r["pass"] == "block" and r["ms"] == 0),
          ("kept = 64, sorted", 0, lambda r: r["kc"] == 64 and r["resolve"] == "sort"),
          ("kept = 65, sorted", 0, lambda r: r["kc"] == 65 and r["resolve"] == "sort")]
    if delta:
        cl += [("kept = 128, sorted", 0, lambda r: r["kc"] == 128 and r["resolve"] == "sort"),
               ("kept = 129, sorted", 0, lambda r: r["kc"] == 129 and r["resolve"] == "sort")]
    return Case("tuple_ladder_" + mode_name(mode), mode, [batches_of(R, docs)], cl)


# ---------------------------------------------------------------- clock ladder

@functools.lru_cache(maxsize=None)
def clock_ladder(mode, per_rung=8):
    """ms * R one source below, at and one above 64, 128, 192 and 256: R = 16 and
    R = 64 (ms = 1..5)."""
    delta = mode == DELTA
    rng = random.Random(9200 + mode)
    out, cl = [], []
    LADDER = ((16, (3, 4, 5, 7, 8, 9, 11, 12, 13, 15, 16, 17)), (64, (1, 2, 3, 4, 5)))
    for R, mss in LADDER:
        docs = []
        for ms in mss:
            for d in range(per_rung):
                base = rng.randrange(0, 1 << 30)
                docs.append(make_doc(rng, R, delta, ms, rng.randint(0, 12), list(range(base, base + 50)),
                                     ents=(0, 4), tombs=(0, 2)))
        out.append(batches_of(R, docs))
    lean_cap, gen_cap = fp.vcap(mode, True), fp.vcap(mode, False)
    for R, mss in LADDER:
        for ms in mss:
            w = ms * R
            for lean in (1, 0):
                if w > gen_cap:
                    p = "block"
                elif not lean:
                    p = "general-direct"
                elif w > lean_cap or ms > fp.T("LEAN_MS"):
                    p = "general-deferred"
                else:
                    continue  # the lean pass takes it, or defers it for another reason
                cl.append(("R=%d ms=%d (%d clock words): %s lean=%d" % (R, ms, w, p, lean), lean,
                           (lambda R, ms, p: lambda r: r["R"] == R and r["ms"] == ms and r["pass"] == p)(R, ms, p)))
    cl.append(("lean defers: clocks", 1, lambda r: r["lean_why"] == "clocks" and r["pass"] == "general-deferred"))
    return Case("clock_ladder_" + mode_name(mode), mode, out, cl)


# ---------------------------------------------------------------- span ladder

def span_doc(rng, R, delta, span, place, wide):
    """Keys of span `span` (max - min): dense -- all tuples within it, the two ends in
    sources (and, delta, a tombstone), dst narrower; wide -- dst holds both ends.
    place: 0 base 0; 1 base 2^63 - 100; 2 ending at 2^64 - 1; 3 wrapping through
    2^64 (the keys are `span` apart modulo 2^64 only: nothing dense about them)."""
    base = (0, (1 << 63) - 100, TOP - span, TOP - span // 2)[place]
    wrap = lambda k: k & TOP  # noqa: E731
    lo, hi = base, base + span
    inner = [base + i for i in range(1, span)]
    ms = rng.randint(2, 6)
    dst, vv, chain = make_doc(rng, R, delta, ms, rng.randint(2, 12), inner, ents=(1, 3), tombs=(0, 2))
    if wide:
        dst = sorted(dst + [(lo,) + dot(rng, R, True), (hi,) + dot(rng, R, True)])
    else:
        a, v, e, t = chain[0]
        chain[0] = (a, v, sorted(e + [(lo,) + dot(rng, R, True)]), t)
        a, v, e, t = chain[-1]
        if delta and rng.random() < 0.5:
            chain[-1] = (a, v, e, sorted([x for x in t if x[0] != hi] + [(hi,) + dot(rng, R, True)]))
        else:
            chain[-1] = (a, v, sorted(e + [(hi,) + dot(rng, R, True)]), t)
    fix = lambda es: sorted((wrap(k), a, c) for k, a, c in es)  # noqa: E731
    return fix(dst), vv, [(a, v, fix(e), fix(t)) for a, v, e, t in chain]


@functools.lru_cache(maxsize=None)
def span_ladder(mode, per=6):
    delta = mode == DELTA
    R = 4
    rng = random.Random(9300 + mode)
    docs = []
    for span in (63, 64, 65, 255, 256, 257):
        for place in range(4):
            for wide in (False, True):
                for _ in range(per):
                    docs.append(span_doc(rng, R, delta, span, place, wide))
    edge = fp.T("SPAN_DELTA") if delta else fp.T("SPAN_AWSET")
    cl = [("lean walks span %d" % (edge - 1), 1, lambda r: r["pass"] == "lean"),
          ("lean defers: span", 1, lambda r: r["lean_why"] == "span" and r["pass"] == "general-deferred"),
          ("general slot walk", 0, lambda r: r["resolve"] == "slot-walk"),
          ("general sort", 0, lambda r: r["resolve"] == "sort")]
    return Case("span_ladder_" + mode_name(mode), mode, [batches_of(R, docs)], cl)


# ---------------------------------------------------------------- document-count ladder

def tiny_doc(d, R, delta):
    """Document d, recognisable: keys 8 d .. 8 d + 3, clocks and counters from d."""
    c = d % 50 + 1
    k = 8 * d
    dst = [(k, d % R, c + 9), (k + 1, (d + 1) % R, 1)]            # the second is removed / kept by the clocks below
    vv = [d % 7 + 1] * R
    s0 = (d % R, [c % 5 + 2] * R, [(k + 2, d % R, c + 10)], [(k + 1, (d + 1) % R, 60)] if delta else [])
    s1 = ((d + 1) % R, [d % 3 + 1] * R, [(k, (d + 1) % R, c + 12), (k + 3, d % R, 1)], [])
    if d % 11 == 7:   # no tuples at all: the lean passes walk no such document
        return [], vv, [(d % R, [1] * R, [], [])] if d % 2 else []
    if d % 5 == 4:    # no sources
        return dst, vv, []
    return dst, vv, [s0, s1]


def deferred_doc(d, R, delta):
    """A document the lean pass defers (16 sources) that stays on the pipe kernels."""
    rng = random.Random(77000 + d)
    return make_doc(rng, R, delta, 16, 5, list(range(8 * d, 8 * d + 8)))


def block_doc(d, R, delta):
    rng = random.Random(78000 + d)
    return sized_doc(rng, R, delta, 200, 100, 20 if delta else 0, 3, list(range(8 * d, 8 * d + 300)))


@functools.lru_cache(maxsize=None)
def doc_count_batch(mode, n_docs, variant, zero_ends=False):
    """n_docs tiny documents; a lean-deferred and a block-path document first, last and
    on both sides of the first run edge (variant 1 swaps the two kinds).  zero_ends:
    instead, the first and the last document have no slots and no sources."""
    delta = mode == DELTA
    R = 2
    K = fp.T("K_DELTA") if delta else fp.T("K_AWSET")
    docs = [tiny_doc(d, R, delta) for d in range(n_docs)]
    if zero_ends:
        docs[0] = ([], [1] * R, [])
        docs[-1] = ([], [2] * R, [])
    else:
        spots = [p for p in (0, K - 1, K, n_docs - 1) if 0 <= p < n_docs]
        for i, p in enumerate(dict.fromkeys(spots)):
            docs[p] = (deferred_doc if (i + variant) % 2 == 0 else block_doc)(p, R, delta)
    return batches_of(R, docs)


@functools.lru_cache(maxsize=None)
def doc_count_ladder(mode):
    batches = [doc_count_batch(mode, n, v) for n in DOC_COUNTS[mode] for v in (0, 1)]
    cl = [("tiny documents in the lean pass", 1, lambda r: r["pass"] == "lean"),
          ("no sources, lean pass", 1, lambda r: r["pass"] == "lean" and r["ms"] == 0),
          ("no tuples: deferred", 1, lambda r: r["why"] == "empty"),
          ("deferred at a run edge", 1, lambda r: r["pass"] == "general-deferred"),
          ("block at a run edge", 1, lambda r: r["pass"] == "block")]
    return Case("doc_count_ladder_" + mode_name(mode), mode, batches, cl)


# ---------------------------------------------------------------- slack

def with_slack(dst_docs, R, rng):
    """(batch with counts and 0..5 slack slots a document, the same documents compact).
    The slack is filled with what would matter if it were read: keys inside the
    document's live range, copies of live keys, actor == R, high counters."""
    n = len(dst_docs)
    counts = np.array([len(e) for e, _ in dst_docs], U32)
    slack = np.array([rng.randint(0, 5) for _ in range(n)], U32)
    off = np.zeros(n + 1, U32)
    np.cumsum(counts + slack, out=off[1:])
    tot = max(int(off[-1]), 1)
    keys, actors, counters = np.zeros(tot, U64), np.zeros(tot, U32), np.zeros(tot, U64)
    vv = np.zeros(n * R, U64)
    for d, (e, v) in enumerate(dst_docs):
        o = int(off[d])
        for i, (k, a, c) in enumerate(e):
            keys[o + i], actors[o + i], counters[o + i] = k, a, c
        live = [k for k, _, _ in e] or [7]
        for i in range(int(slack[d])):
            s = o + len(e) + i
            keys[s] = (rng.choice(live), (min(live) + max(live)) // 2, min(live))[i % 3]
            actors[s] = R if i % 2 == 0 else rng.randrange(R)
            counters[s] = CMAX
        vv[d * R:(d + 1) * R] = v
    return (AWSetBatch(R, off, keys, actors, counters, vv, counts),
            AWSetBatch.from_docs(R, dst_docs))


@functools.lru_cache(maxsize=None)
def slack_case(mode, n_docs=150):
    """(Case over the slack batch, the compact twin's dst)."""
    delta = mode == DELTA
    R = 3
    rng = random.Random(9500 + mode)
    docs = []
    for d in range(n_docs):
        ms = (3, 9, 16, 40, 2)[d % 5]
        nd = 140 if d % 25 == 7 else rng.randint(0, 20)  # a few on the block path
        docs.append(make_doc(rng, R, delta, ms, nd, list(range(100 * d, 100 * d + (200 if nd > 60 else 45)))))
    slack, compact = with_slack([(e, vv) for e, vv, _ in docs], R, rng)
    srcs = SrcBatch.from_lists(R, [c for _, _, c in docs])
    cl = [("slack: lean", 1, lambda r: r["pass"] == "lean"),
          ("slack: general", 0, lambda r: r["pass"] == "general-direct")]
    return Case("slack_" + mode_name(mode), mode, [(slack, srcs)], cl), compact


# ---------------------------------------------------------------- no tombstone arrays

@functools.lru_cache(maxsize=None)
def no_tomb_case(n_docs=120):
    """A delta source batch with tomb_off == NULL, and its twin with empty ranges."""
    R = 3
    rng = random.Random(9600)
    docs = []
    for d in range(n_docs):
        ms = (2, 7, 15, 16, 33)[d % 5]
        feature = (None, "first", "noop")[d % 3]
        docs.append(make_doc(rng, R, True, ms, rng.randint(0, 20), list(range(64 * d, 64 * d + 40)), ents=(1, 3),
                             tombs=(0, 0), feature=feature, p_hi=0.8))
    dst, twin = batches_of(R, docs)
    bare = SrcBatch(R, twin.doc_srcs, twin.src_actor, twin.vv, twin.entry_off, twin.keys, twin.actors, twin.counters)
    cl = [("no tombstones: lean", 1, lambda r: r["pass"] == "lean"),
          ("no tombstones: deferred", 1, lambda r: r["pass"] == "general-deferred")]
    return Case("no_tombs_delta", DELTA, [(dst, bare)], cl), twin


# ---------------------------------------------------------------- actor == len(VV), never evaluated

@functools.lru_cache(maxsize=None)
def actor_edge_case(n_docs=24):
    """Delta folds whose documents hold an entry of actor == R that the reference never
    looks at (no full step: a delta step compares the clock with the source's dots
    only), so the fold succeeds; the lean pass leaves such a document to the sort path."""
    R = 3
    rng = random.Random(9700)
    docs = []
    for d in range(n_docs):
        dst, vv, chain = make_doc(rng, R, True, rng.randint(1, 9), rng.randint(1, 10), list(range(50 * d, 50 * d + 30)))
        dst = sorted(dst + [(50 * d + 40, R, rng.randint(1, CMAX))])
        docs.append((dst, vv, chain))
    cl = [("lean defers: actor == R", 1, lambda r: r["lean_why"] == "actor==R")]
    return Case("actor_edge_delta", DELTA, [batches_of(R, docs)], cl)


@functools.lru_cache(maxsize=None)
def actor_edge_awset(n_docs=24):
    """AWSet folds of documents holding an entry of actor == R whose key the first source
    holds too: its dot is replaced before any clock is asked about it, so the fold
    succeeds, through the slot walk's step-by-step form."""
    R = 3
    rng = random.Random(9701)
    docs = []
    for d in range(n_docs):
        dst, vv, chain = make_doc(rng, R, False, rng.randint(1, 9), rng.randint(1, 10), list(range(50 * d, 50 * d + 30)))
        k = 50 * d + 40
        a, v, e, t = chain[0]
        chain[0] = (a, v, sorted(e + [(k,) + dot(rng, R, True)]), t)
        docs.append((sorted(dst + [(k, R, rng.randint(1, CMAX))]), vv, chain))
    cl = [("slot walk, step by step", 1, lambda r: r["pass"] == "lean" and r["seq_walk"])]
    return Case("actor_edge_awset", AWSET, [batches_of(R, docs)], cl)


# ---------------------------------------------------------------- all of them

_cases = None


def all_cases():
    """Every case, built once (never modified by a test)."""
    global _cases
    if _cases is None:
        cs = []
        for mode in MODES:
            cs += [source_ladder(mode, R) for R in LADDER_R[mode]]
            cs += [tuple_ladder(mode), clock_ladder(mode), span_ladder(mode), doc_count_ladder(mode),
                   slack_case(mode)[0]]
        cs += [no_tomb_case()[0], actor_edge_case(), actor_edge_awset()]
        _cases = {c.name: c for c in cs}
    return _cases
