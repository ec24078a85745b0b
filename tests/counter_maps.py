"""Order-preserving counter maps: small-counter cases pushed up to the 32- and
64-bit edges of the ABI's u64 dot counters and clocks.

AWSet join, the ordered AWSet / AWSetDelta folds, delta extraction and the
tombstone GC use counters only through >=, >, ==, max and "is the clock entry
0" (awset.go:103-161, awset-delta_test.go:35-102, crdt-misc.go:24-55).  For a
strictly increasing f with f(0) = 0

    op(f(inputs)) == f(op(inputs))

bit for bit: slot bounds, counts, keys, actors and error verdicts unchanged,
every counter and clock value of the output f of the unmapped one.  So a
small-counter case mapped through f is a wide-counter case on the same kernel
path with two independent expectations (the oracle on the mapped inputs, and
the mapped result of the unmapped run).  tests/test_counter_maps_model.py shows
the property on the oracles; tests/test_gpu_wide_counters.py uses it on the
kernels.  The local ops (apply) do arithmetic on the clock and are not covered
by it.

A table is a numpy u64 array t with t[c] = f(c) over 0..C.  The generators the
GPU tests reuse draw counters from 1..max_c with max_c between 6 and 50;
stretch() spreads that range over the whole table first (itself a strictly
increasing map), so that a case with counters 1..9 still lands on both sides
of a table's edge and reaches its top value.
"""

from __future__ import annotations

import random
from typing import Callable, NamedTuple

import numpy as np

from crdtgpu.batch import AWSetBatch, OutBuffers, SrcBatch, TombBatch

U64 = np.uint64
C = 64
TOP = (1 << 64) - 1


class CounterMap(NamedTuple):
    name: str
    table: np.ndarray  # u64 [C + 1], strictly increasing, table[0] == 0
    edge: int          # the boundary the map is about: outputs must reach values >= edge


def _table(f) -> np.ndarray:
    return np.array([0] + [f(c) for c in range(1, C + 1)], dtype=U64)


def _scattered():
    rng = random.Random(0xC0FFEE)
    vals = set()
    while len(vals) < C:
        v = rng.getrandbits(64)
        if v:
            vals.add(v)
    return sorted(vals)


_SC = _scattered()

# name, f(c) for c >= 1, and what a kernel that gets it wrong would do
MAPS = [
    # comparisons or moves that see only the low word: all equal
    CounterMap("hi_only", _table(lambda c: c << 32), 1 << 32),
    # low-word-only order inverts at the wrap; high-word-only ties on either side
    CounterMap("across_2_32", _table(lambda c: (1 << 32) - 32 + c), 1 << 32),
    # a signed 32-bit compare (every value fits 32 bits: the edge is bit 31, not the high word)
    CounterMap("across_2_31", _table(lambda c: (1 << 31) - 32 + c), 1 << 31),
    # a signed 64-bit compare
    CounterMap("across_2_63", _table(lambda c: (1 << 63) - 32 + c), 1 << 63),
    # the maximum 2^64 - 1: ~0ull sentinels, saturation
    CounterMap("top", _table(lambda c: TOP - C + c), TOP - C + 1),
    # halves swapped or mixed between lanes
    CounterMap("scattered", _table(lambda c: _SC[c - 1]), 1 << 32),
]

_stretched = {}
_owner = {id(m.table): m.name for m in MAPS}  # table (by identity; all are kept alive here) -> its map's name


def stretch(m: CounterMap, max_c: int) -> np.ndarray:
    """The table of c -> m.table[c * C // max_c] over 0..max_c (max_c <= C): the
    generator's counter range spread over the whole table, max_c on its top."""
    assert 1 <= max_c <= C
    key = (m.name, max_c)
    if key not in _stretched:
        _stretched[key] = m.table[np.arange(max_c + 1) * C // max_c]
        _owner[id(_stretched[key])] = m.name
    return _stretched[key]


def mixed(max_c: int = C, period: int = 0) -> Callable[[int], np.ndarray]:
    """table_of_doc giving document d the map MAPS[d % 6], stretched from 0..max_c.
    period: the generator's own cycle over d (kinds of document, key maps); the
    map then also advances once per cycle, so that every kind meets every map."""
    if period:
        return lambda d: stretch(MAPS[(d + d // period) % len(MAPS)], max_c)
    return lambda d: stretch(MAPS[d % len(MAPS)], max_c)


def single(m: CounterMap, max_c: int = C) -> Callable[[int], np.ndarray]:
    return lambda d: stretch(m, max_c)


def map_name(table) -> str:
    """The name of the map a table (of MAPS or of stretch()) belongs to."""
    return _owner[id(table)]


# ---------------------------------------------------------------- appliers

def _tables(table_of_doc, n_docs):
    """(stacked distinct tables padded to one width, table index per doc)."""
    seen, tabs, idx = {}, [], np.zeros(n_docs, dtype=np.int64)
    for d in range(n_docs):
        t = table_of_doc(d)
        if id(t) not in seen:
            seen[id(t)] = len(tabs)
            tabs.append(t)
        idx[d] = seen[id(t)]
    lens = np.array([len(t) for t in tabs] or [0], dtype=np.int64)
    stack = np.zeros((max(len(tabs), 1), int(lens.max())), dtype=U64)
    for i, t in enumerate(tabs):
        stack[i, : len(t)] = t
    return stack, lens, idx


def _live(offsets, counts):
    """(slot index, doc index) of every live slot of a batch."""
    o = np.asarray(offsets).astype(np.int64)
    n = len(o) - 1
    cnt = (o[1:] - o[:-1]) if counts is None else np.asarray(counts)[:n].astype(np.int64)
    doc = np.repeat(np.arange(n), cnt)
    slot = np.repeat(o[:-1], cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return slot, doc


def _apply(values, slot, doc, tabs):
    """A copy of `values` with values[slot] looked up in the table of its doc.  A
    value outside its table is an error (the case is not the small-counter case
    it was taken for), never silently passed through."""
    stack, lens, idx = tabs
    out = np.array(values, dtype=U64, copy=True)
    if len(slot):
        t = idx[doc]
        v = out[slot]
        assert (v < lens[t].astype(U64)).all(), "counter outside its table"
        out[slot] = stack[t, v.astype(np.int64)]
    return out


def _map_vv(vv, n_rows, R, row_doc, tabs):
    rows = np.repeat(np.asarray(row_doc, dtype=np.int64), R)
    return _apply(vv, np.arange(n_rows * R), rows, tabs)


def map_batch(batch, table_of_doc):
    """An AWSetBatch (counters of live entries, clocks) or a TombBatch (tombstone
    counters) with every document's values through its table.  Keys, actors,
    offsets and counts are shared with the input."""
    n = batch.n_docs
    tabs = _tables(table_of_doc, n)
    slot, doc = _live(batch.offsets, batch.counts)
    counters = _apply(batch.counters, slot, doc, tabs)
    if isinstance(batch, TombBatch):
        return TombBatch(batch.offsets, batch.keys, batch.actors, counters, batch.counts)
    vv = _map_vv(batch.vv, n, batch.R, np.arange(n), tabs)
    return AWSetBatch(batch.R, batch.offsets, batch.keys, batch.actors, counters, vv, batch.counts)


def map_srcs(srcs: SrcBatch, table_of_doc) -> SrcBatch:
    """A SrcBatch (fold sources, or an extracted message) with every source's
    clock, entry counters and tombstone counters through its document's table.
    Only the slots below entry_off[n_srcs] / tomb_off[n_srcs] are entries."""
    n = srcs.n_docs
    tabs = _tables(table_of_doc, n)
    ds = np.asarray(srcs.doc_srcs).astype(np.int64)
    ns = int(ds[-1])
    src_doc = np.repeat(np.arange(n), ds[1:] - ds[:-1])
    vv = _map_vv(srcs.vv, ns, srcs.R, src_doc, tabs)

    def col(off, values):
        if off is None or values is None:
            return values
        slot, s = _live(np.asarray(off)[: ns + 1], None)
        return _apply(values, slot, src_doc[s], tabs)

    return SrcBatch(srcs.R, srcs.doc_srcs, srcs.src_actor, vv, srcs.entry_off, srcs.keys, srcs.actors,
                    col(srcs.entry_off, srcs.counters), srcs.tomb_off, srcs.tkeys, srcs.tactors,
                    col(srcs.tomb_off, srcs.tcounters))


def map_out(out, table_of_doc):
    """A join / fold output (OutBuffers), a tombstone output (TombBatch) or an
    extracted message (SrcBatch) with the live counters and the clocks through
    each document's table; slots past a document's count stay as they are."""
    if isinstance(out, SrcBatch):
        return map_srcs(out, table_of_doc)
    if isinstance(out, TombBatch):
        return map_batch(out, table_of_doc)
    n, R = out.n_docs, out.R
    tabs = _tables(table_of_doc, n)
    slot, doc = _live(np.asarray(out.offsets)[: n + 1], out.counts)
    m = OutBuffers(n, R, 0)
    m.offsets, m.counts, m.keys, m.actors = out.offsets, out.counts, out.keys, out.actors
    m.counters = _apply(out.counters, slot, doc, tabs)
    m.vv = _map_vv(np.asarray(out.vv)[: n * R], n, R, np.arange(n), tabs)
    return m


def map_clocks(vv, R, table_of_doc):
    """A flat [n_docs * R] clock array (peer clocks, stable clocks) through the tables."""
    vv = np.asarray(vv, dtype=U64).reshape(-1)
    n = len(vv) // R
    return _map_vv(vv, n, R, np.arange(n), _tables(table_of_doc, n))


# list forms, for the restatements that work on Python lists

def map_entries(ents, t):
    return None if ents is None else [(k, a, int(t[c])) for k, a, c in ents]


def map_clock(vv, t):
    return [int(t[v]) for v in vv]


def map_source_lists(per_doc, table_of_doc):
    """per_doc[d] = [(actor, vv, entries, tombstones or None)] through the tables."""
    return [[(a, map_clock(vv, table_of_doc(d)), map_entries(e, table_of_doc(d)), map_entries(tb, table_of_doc(d)))
             for a, vv, e, tb in sources] for d, sources in enumerate(per_doc)]


# ---------------------------------------------------------------- the case-mix condition

def assert_mixes(out, table_of_doc, what=""):
    """The output of a case (the oracle's, so this is a condition on the case and
    can be checked without a GPU) really is a wide-counter one under every map:
    the batch's documents use all of MAPS, and for each map some live output
    counter or clock value lies at or above the map's edge -- a non-zero high
    word, or for across_2_31, whose values fit 32 bits by construction, bit 31."""
    if isinstance(out, SrcBatch):
        n = out.n_docs
        ds = np.asarray(out.doc_srcs).astype(np.int64)
        ns = int(ds[-1])
        src_doc = np.repeat(np.arange(n), ds[1:] - ds[:-1])
        _, s = _live(np.asarray(out.entry_off)[: ns + 1], None)
        vals = np.asarray(out.counters)[: len(s)]
        docs = src_doc[s]
        if out.tomb_off is not None:
            _, s2 = _live(np.asarray(out.tomb_off)[: ns + 1], None)
            vals = np.concatenate([vals, np.asarray(out.tcounters)[: len(s2)]])
            docs = np.concatenate([docs, src_doc[s2]])
    else:
        n = out.n_docs
        slot, docs = _live(np.asarray(out.offsets)[: n + 1], out.counts)
        vals = np.asarray(out.counters)[slot]
        if hasattr(out, "vv") and getattr(out, "R", 0):
            vals = np.concatenate([vals, np.asarray(out.vv)[: n * out.R]])
            docs = np.concatenate([docs, np.repeat(np.arange(n), out.R)])
    vals = vals.astype(U64)
    names = {}
    for d in range(n):
        names.setdefault(_owner[id(table_of_doc(d))], []).append(d)
    assert set(names) == {m.name for m in MAPS}, (what, "maps in the batch", sorted(names))
    for m in MAPS:
        v = vals[np.isin(docs, names[m.name])]
        assert (v >= U64(m.edge)).any(), (what, m.name, "no output value at or above the edge")
