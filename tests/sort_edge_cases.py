"""Deterministic cases that sit on every edge of the ingest sort (csrc/sort.hip, wave_sort_pairs
in csrc/wave_sort.hpp) and of the device order check (check_order_kernel, csrc/pack.hip).

The sort gives a document of n <= 256 live entries to one wavefront: EPL = 1, 2 or 4 entries a
lane (n <= 64, <= 128, <= 256), element i in lane i / EPL, slot i % EPL.  wave_sort_pairs takes
every key by its offset from b, the first key in input order, and picks the compare width from
those offsets: 32-bit packed for offsets in [-2^15, 2^15), 64-bit packed for [-2^47, 2^47), the
80-bit (key, index) compare otherwise, and always when the keys are that close only modulo 2^64.
A larger document goes to one workgroup: 256-entry runs sorted as above (each run's b is its own
first element), then merge-path passes that double the run length, 8 outputs a thread, the keys
ping-ponging between two buffers.  A repeated key is found next to its twin after the sort; on the
wave path a lane's first element is compared with the previous lane's last through a DPP shift.

The order check gives each range (a document, a source's entries, a source's tombstones) to a
wavefront; lane l compares pair (i - 1, i) for i = 1 + l, 65 + l, ...

Each Case puts one of those quantities on a boundary; `claims` names the edge in quantities
`census` recomputes from the case alone, so tests/test_sort_edges_model.py fails when a case
drifts off its edge.  No RNG, no GPU: every permutation is one of the closed forms below.  A key
is a Python int; an entry's dot is a function of its key (and of which copy of a repeated key it
is, in input order), so a misplaced dot shows.
"""

from __future__ import annotations

from math import gcd
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from crdtgpu import CRDT_E_CAPACITY, CRDT_E_DUP_KEY, CRDT_E_UNSORTED
from crdtgpu.batch import AWSetBatch, SrcBatch

U32, U64 = np.uint32, np.uint64
M64 = 1 << 64
TOP = M64 - 1
WAVE_MAX = 256       # sort.hip: kSortWaveMax
ITEMS = 8            # sort.hip: kSortItems
ORDER_LANES = 64     # pack.hip: check_order_kernel's stride
OVER = 9             # an over-count document claims this many entries above its slots
B0 = (1 << 52) + 0x1234  # the first key of the threshold documents: B0 +- 2^47 +- 1 stays inside the key range
FILLS = ("zeros", "ones", "continuation")

Entry = Tuple[int, int, int]
Doc = Tuple[List[Entry], List[int]]


class Case(NamedTuple):
    name: str
    group: str
    R: int
    docs: List[Doc]                     # every document's live entries in input order, and its clock
    slack: Tuple[int, ...]              # spare slots after each document
    claims: Dict[str, object]           # census quantities of document claims["at"] (default 0)
    want: Optional[int] = None          # None: the reference sort; else the error code
    over: Optional[Tuple[int, int]] = None  # (document, n): its count is its slots + n
    twin: Optional[str] = None          # a dup case's clean twin


class OrderCase(NamedTuple):
    name: str
    R: int
    docs: List[Doc]                     # live entries as the merge kernels get them (a violation included)
    slack_rows: List[List[Entry]]       # what each document's spare slots hold
    counted: bool                       # counts given; False: a range ends at the next offset (no slack)
    srcs: Optional[list]                # fold form: per document [(actor, clock, entries, tombstones)]
    claims: Dict[str, object]
    want: int                           # CRDT_OK or CRDT_E_UNSORTED, stated by hand


# ------------------------------------------------------------------ entries, permutations

def dot(k, R, occ=0):
    """The dot of key k (copy `occ` of it): actor below R, counter odd-spread over 64 bits, never 0."""
    return (k ^ (k >> 17)) % R, ((k * 0x9E3779B97F4A7C15) % (1 << 62)) * 4 + occ + 1


def entries(keys, R):
    seen, out = {}, []
    for k in keys:
        assert 0 <= k <= TOP
        out.append((k,) + dot(k, R, seen.get(k, 0)))
        seen[k] = seen.get(k, 0) + 1
    return out


def clock(d, R):
    return [131 * d + 7 * r + 1 for r in range(R)]


def identity(n):
    return list(range(n))


def reversal(n):
    return [n - 1 - i for i in range(n)]


def rotation(n):
    """Rotation by one: the last key first."""
    return [(i - 1) % n for i in range(n)]


def first_last(n):
    """The first key last."""
    return list(range(1, n)) + [0] if n else []


def mult(n):
    """An odd multiplier near 5n/8 coprime to n."""
    a = max(1, (5 * n) // 8) | 1
    while gcd(a, n) != 1:
        a += 2
    return a


def affine(n, c=0, a=None):
    """i -> (a i + c) mod n."""
    a = mult(n) if a is None else a
    assert n == 0 or gcd(a, n) == 1
    return [(a * i + c) % n for i in range(n)]


def permuted(s, perm):
    assert sorted(perm) == list(range(len(s)))
    return [s[p] for p in perm]


def case(name, group, key_lists, claims, R=3, slack=None, want=None, over=None, twin=None):
    docs = [(entries(keys, R), clock(d, R)) for d, keys in enumerate(key_lists)]
    return Case(name, group, R, docs, tuple(slack) if slack else (0,) * len(docs), claims, want, over, twin)


# ------------------------------------------------------------------ the selection model and the census

def epl_of(n):
    return 1 if n <= 64 else 2 if n <= 128 else 4


def width_of(run):
    """The compare width wave_sort_pairs picks for the live keys `run` (input order): u64 arithmetic restated."""
    b = run[0]
    o16 = o48 = False
    for k in run:
        d = (k - b) % M64
        neg = d >= 1 << 63
        wrap = (k < b) != neg
        o16 |= wrap or (d + 0x8000) % M64 >= 0x10000
        o48 |= wrap or (d + (1 << 47)) % M64 >= 1 << 48
    return 32 if not o16 else 64 if not o48 else 80


def live_keys(c: Case, d):
    """The keys the kernel takes as document d's live ones: an over-count is clamped to the
    slots, which then hold the live entries and nothing else (an over-count document has no slack)."""
    return [k for k, _, _ in c.docs[d][0]]


def census(c: Case):
    at = c.claims.get("at", 0)
    keys = live_keys(c, at)
    n = len(keys)
    path = "wave" if n <= WAVE_MAX else "block"
    runs = [keys[i:i + WAVE_MAX] for i in range(0, n, WAVE_MAX)] if n else []
    s = sorted(keys)
    epl = epl_of(n) if path == "wave" else 4
    dups = []
    for i in range(1, n):
        if s[i] == s[i - 1]:
            dups.append((i - 1, i) + ((i // epl, i % epl) if path == "wave" else (i // ITEMS, i % ITEMS)))
    where = {}
    for i, k in enumerate(keys):
        where.setdefault(k, []).append(i // WAVE_MAX)
    out = dict(at=at, n=n, epl=epl, path=path, runs=max(1, len(runs)), passes=max(0, len(runs) - 1).bit_length(),
               widths=[width_of(r) for r in runs], offs=[(min(r) - r[0], max(r) - r[0]) for r in runs], dups=dups,
               dup_key=s[dups[0][1]] if dups else None, first=keys[0] if keys else None,
               dup_runs=sorted(set(tuple(v) for v in where.values() if len(v) > 1)))
    if c.over:
        d, above = c.over
        cnt = len(c.docs[d][0]) + c.slack[d] + above
        out["unclamped_path"] = "wave" if cnt <= WAVE_MAX else "block"
    return out


def order_census(c: OrderCase):
    """The first violating pair (i - 1, i) of document claims["at"] and the lane that checks it."""
    at = c.claims.get("at", 1)
    keys = [k for k, _, _ in c.docs[at][0]]
    bad = [i for i in range(1, len(keys)) if keys[i] <= keys[i - 1]]
    return dict(at=at, m=len(keys), pair=(bad[0] - 1, bad[0]) if bad else None,
                lane=(bad[0] - 1) % ORDER_LANES if bad else None, step=(bad[0] - 1) // ORDER_LANES if bad else None,
                n_bad=len(bad))


# ------------------------------------------------------------------ batches

def pack(docs, R, slacks, fill="zeros", over=None, rows=None, counted=None):
    """An AWSetBatch of docs with slacks[d] spare slots after document d, filled by `fill` (or
    holding rows[d]); over = (document, count).  counts is None where nothing needs it."""
    n = len(docs)
    live = np.array([len(e) for e, _ in docs], dtype=np.int64)
    caps = live + np.array(slacks, dtype=np.int64).reshape(n)
    offsets = np.zeros(n + 1, dtype=U32)
    np.cumsum(caps, out=offsets[1:])
    total = int(offsets[-1])
    keys, actors, counters = np.zeros(max(total, 1), U64), np.zeros(max(total, 1), U32), np.zeros(max(total, 1), U64)
    vv = np.zeros(max(n * R, 1), U64)
    for d, (ents, v) in enumerate(docs):
        o = int(offsets[d])
        row = list(ents)
        if rows is not None:
            assert len(rows[d]) == slacks[d]
            row += rows[d]
        elif fill == "ones":
            row += [(TOP, 0xFFFFFFFF, TOP)] * slacks[d]
        elif fill == "continuation":  # more entries of the same kind: keys on from the last one in input order
            last = ents[-1][0] if ents else 0
            row += entries([(last + 1 + i) % M64 for i in range(slacks[d])], R)
        for i, (k, a, c) in enumerate(row):
            keys[o + i], actors[o + i], counters[o + i] = k, a, c
        vv[d * R:(d + 1) * R] = v
    counts = live.astype(U32)
    if over is not None:
        counts[over[0]] = over[1]
    if counted is None:
        counted = over is not None or any(slacks)
    return AWSetBatch(R, offsets, keys, actors, counters, vv[: n * R] if n else vv[:0], counts if counted else None)


def batch_of(c: Case, extra=0, fill="zeros"):
    """The case as the kernel gets it (an over-count case with its bad count)."""
    over = None
    if c.over:
        assert extra == 0
        d, above = c.over
        assert c.slack[d] == 0, "an over-count document has no slack: its clamped prefix is its live entries"
        over = (d, len(c.docs[d][0]) + above)
    return pack(c.docs, c.R, [s + extra for s in c.slack], fill, over)


def concat(cases, extra=0, fill="zeros"):
    """One batch of the documents of all `cases` (equal R, none over-count) and the first document of each."""
    docs, slacks, first = [], [], []
    for c in cases:
        assert c.over is None and c.R == cases[0].R
        first.append(len(docs))
        docs += c.docs
        slacks += [s + extra for s in c.slack]
    return pack(docs, cases[0].R, slacks, fill, counted=True), first


def reference(c: Case):
    """Per document: (entries sorted, clock).  Python's sorted on int tuples; a repeated key's
    copies stay in input order (the sort is stable: every compare is on (key, input index))."""
    out = []
    for ents, v in c.docs:
        order = sorted(range(len(ents)), key=lambda i: (ents[i][0], i))
        want = [ents[i] for i in order]
        if len({k for k, _, _ in ents}) == len(ents):
            assert want == sorted(ents)
        out.append((want, list(v)))
    return out


# ------------------------------------------------------------------ 1. width: the thresholds

THRESHOLDS = {  # offset of one key from b: the width it forces
    "m8000": (-0x8000, 32), "m8001": (-0x8001, 64), "p7fff": (0x7FFF, 32), "p8000": (0x8000, 64),
    "m2_47": (-(1 << 47), 64), "m2_47_1": (-(1 << 47) - 1, 80), "p2_47_1": ((1 << 47) - 1, 64), "p2_47": (1 << 47, 80),
}


def near(b, m):
    """m keys around b: b + 1, b - 1, b + 2, ... (within +-100 of b up to 200 keys)."""
    out, j = [], 1
    while len(out) < m:
        out += [b + j, b - j][: m - len(out)]
        j += 1
    return out


def run_with(b, m, t=None, p=None):
    """A run of m keys in input order: b first, the others near b, key t at element p."""
    if t is None:
        return [b] + near(b, m - 1)
    rest = near(b, m - 2)
    return [b] + rest[: p - 1] + [t] + rest[p - 1:]


def width_cases():
    out = []
    for tname, (off, w) in THRESHOLDS.items():
        for n in (40, 100, 200):
            full = epl_of(n) * 64
            for place, m, p in (("elem1", n, 1), ("last_live", n, n - 1), ("last_slot", full, full - 1)):
                keys = run_with(B0, m, B0 + off, p)
                lo, hi = min(off, -((m - 1) // 2)), max(off, (m - 1) // 2)
                out.append(case("width_%s_n%d_%s" % (tname, n, place), "width", [keys],
                                dict(n=m, epl=epl_of(n), path="wave", widths=[w], threshold=tname, place=place,
                                     offs=[(lo, hi)])))
        b1 = B0 + (1 << 21)
        for place, n, r, p in (("run0_elem1", 300, 0, 1), ("run0_last_slot", 300, 0, 255), ("run1_elem1", 300, 1, 1),
                               ("run1_last_live", 300, 1, 43), ("run1_last_slot", 512, 1, 255)):
            r0 = run_with(B0, 256, B0 + off, p) if r == 0 else run_with(B0, 256)
            r1 = run_with(b1, n - 256, b1 + off, p) if r == 1 else run_with(b1, n - 256)
            out.append(case("width_%s_n%d_%s" % (tname, n, place), "width", [r0 + r1],
                            dict(n=n, epl=4, path="block", runs=2, passes=1, widths=[w, 32] if r == 0 else [32, w],
                                 threshold=tname, place=place, run=r)))
    return out


# ------------------------------------------------------------------ 2. the ends of the key range

FAR = {32: [], 64: [1 << 20]}  # an extra offset that takes the document out of the 32-bit band


def range_end_cases():
    out = []
    for w in (32, 64):
        for n in (8, 100, 200):
            # b = 3, keys down to 0: the rebuild b - 2^15 (b - 2^47) + offset wraps through 2^64 by design
            keys = [3, 1, 0, 2] + [4 + i for i in range(n - 4 - len(FAR[w]))] + [3 + f for f in FAR[w]]
            out.append(case("low_end_w%d_n%d" % (w, n), "range_ends", [keys], dict(n=n, epl=epl_of(n), widths=[w], first=3)))
        for epl in (1, 2, 4):
            for n in (epl * 64 - 1, epl * 64):
                # b = 2^64 - 3, keys up to 2^64 - 1, a valid key equal to the pad key; with a pad (n odd) and without
                b = TOP - 2
                keys = [b, TOP, TOP - 1] + [b - 1 - i for i in range(n - 3 - len(FAR[w]))] + [b - f for f in FAR[w]]
                out.append(case("top_end_w%d_n%d" % (w, n), "range_ends", [keys],
                                dict(n=n, epl=epl, widths=[w], first=b, pads=epl * 64 - n)))
    # close only modulo 2^64: the offsets would pack, the order across the wrap would be wrong
    for name, keys in (("wrap_b2_top", [2, 5, TOP - 1, 3]), ("wrap_btop_2", [TOP - 1, TOP - 4, 2, TOP - 2]),
                       ("wrap_b2_far", [2, 5, M64 - (1 << 20), 3]), ("wrap_bfar_2", [M64 - (1 << 20), 2, M64 - (1 << 20) + 9]),
                       ("wrap_b0_top", [0, TOP]), ("wrap_btop_0", [TOP, 0])):
        out.append(case(name, "range_ends", [keys], dict(n=len(keys), widths=[80], path="wave")))
    out.append(case("top_alone", "range_ends", [[TOP]], dict(n=1, widths=[32], first=TOP)))
    out.append(case("empty_alone", "range_ends", [[]], dict(n=0, widths=[])))
    out.append(case("zero_alone", "range_ends", [[0]], dict(n=1, widths=[32], first=0)))
    return out


# ------------------------------------------------------------------ 3. sizes of the wave path

WAVE_SIZES = (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256)
ORDERS = {"sorted": identity, "reversed": reversal, "permuted": affine, "rotated": rotation, "first_last": first_last}


def size_cases():
    out = []
    for n in WAVE_SIZES:
        s = [1000 + 3 * i for i in range(n)]
        for order in ("sorted", "reversed", "permuted"):
            out.append(case("size_%d_%s" % (n, order), "sizes", [permuted(s, ORDERS[order](n))],
                            dict(n=n, epl=epl_of(n), path="wave", order=order)))
    for order in ("rotated", "first_last"):
        s = [1000 + 3 * i for i in range(100)]
        out.append(case("size_100_%s" % order, "sizes", [permuted(s, ORDERS[order](100))], dict(n=100, order=order)))
    full = permuted([50 + 2 * i for i in range(64)], affine(64))
    out.append(case("empty_between_two_full", "sizes", [full, [], full], dict(at=1, n=0)))
    return out


# ------------------------------------------------------------------ 4. the block path

BLOCK_SIZES = (257, 263, 511, 512, 513, 768, 769, 1024, 1025, 2048, 2049)
PATTERNS = ("sorted", "reversed", "runs_descend", "runs_ascend", "interleaved", "ends")


def run_sizes(n):
    return [min(WAVE_MAX, n - b) for b in range(0, n, WAVE_MAX)]


def block_keys(n, pattern):
    s = [7 + 5 * i for i in range(n)]
    sizes = run_sizes(n)
    if pattern == "sorted":
        return s
    if pattern == "reversed":
        return s[::-1]
    if pattern == "runs_descend":  # run r entirely above run r + 1, each run ascending
        out, hi = [], n
        for m in sizes:
            out += s[hi - m:hi]
            hi -= m
        return out
    if pattern == "runs_ascend":  # run r entirely below run r + 1, each run descending
        out, lo = [], 0
        for m in sizes:
            out += s[lo:lo + m][::-1]
            lo += m
        return out
    if pattern == "interleaved":  # rank i goes to the runs in turn, while they have room
        runs = [[] for _ in sizes]
        r = 0
        for k in s:
            while len(runs[r]) == sizes[r]:
                r = (r + 1) % len(sizes)
            runs[r].append(k)
            r = (r + 1) % len(sizes)
        return [k for run in runs for k in run]
    assert pattern == "ends"  # 0 and 2^64 - 1 (the merge's own sentinel) present, the rest spread over the key range
    s = [0] + [(i * (M64 // n)) | 1 for i in range(1, n - 1)] + [TOP]
    return permuted(s, affine(n))


def block_cases():
    out = []
    for n in BLOCK_SIZES:
        runs = len(run_sizes(n))
        for pattern in PATTERNS:
            out.append(case("block_%d_%s" % (n, pattern), "block", [block_keys(n, pattern)],
                            dict(n=n, path="block", runs=runs, passes=(runs - 1).bit_length(), pattern=pattern,
                                 odd_run_alone=runs % 2 == 1)))
    return out


# ------------------------------------------------------------------ 5. repeated keys

def keyset(width, n):
    if width == 32:
        return [B0 + 3 * i for i in range(n)]
    if width == 64:
        return [B0 + (i << 20) for i in range(n)]
    assert n < 1024
    return [(i << 54) + 5 for i in range(n)]


def dup_positions(n):
    """The second index of every listed pair of sorted positions."""
    if n > WAVE_MAX:
        return {"first": 1, "last": n - 1, "run_edge": 256, "unit_edge": 8, "second_run_edge": 512}
    epl = epl_of(n)
    pos = {"first": 1, "last": n - 1, "row15_16": 16 * epl, "row31_32": 32 * epl, "row47_48": 48 * epl}
    if epl > 1:
        pos["lane0_1"] = epl
    return pos


DUP_SIZES = (61, 125, 253, 600)


def dup_pair(name, s, copies, perm, claims):
    """(the dup case, its clean twin): s sorted and distinct; copies: positions that repeat the key before them."""
    dup = list(s)
    for i in copies:
        dup[i] = dup[i - 1]
    twin = "%s_twin" % name
    return [case(name, "dup", [permuted(dup, perm)], claims, want=CRDT_E_DUP_KEY, twin=twin),
            case(twin, "dup_twin", [permuted(s, perm)], dict(n=len(s), widths=claims["widths"]))]


def dup_cases():
    out = []
    for n in DUP_SIZES:
        runs = len(run_sizes(n))
        for w in (32, 64, 80):
            for pname, i in dup_positions(n).items():
                s = keyset(w, n)
                out += dup_pair("dup_w%d_n%d_%s" % (w, n, pname), s, [i], affine(n),
                                dict(n=n, widths=[w] * runs, pair=(i - 1, i), path="wave" if n <= WAVE_MAX else "block"))
    for n in (61, 253, 600):
        runs = len(run_sizes(n))
        zero = [3 * i for i in range(n)]
        out += dup_pair("dup_zero_n%d" % n, zero, [1], affine(n), dict(n=n, widths=[32] * runs, pair=(0, 1), dup_key=0))
        top = [TOP - 3 * (n - 1 - i) for i in range(n)]
        out += dup_pair("dup_top_n%d" % n, top, [n - 1], affine(n),
                        dict(n=n, widths=[32] * runs, pair=(n - 2, n - 1), dup_key=TOP - 3))
        s = keyset(32, n)
        out += dup_pair("dup_triple_n%d" % n, s, [n // 2, n // 2 + 1], affine(n), dict(n=n, widths=[32] * runs, triple=n // 2))
    for w in (32, 64, 80):  # the repeated key is b, the first key in input order
        s = keyset(w, 100)
        out += dup_pair("dup_is_b_w%d" % w, s, [41], affine(100, c=40), dict(n=100, widths=[w], pair=(40, 41), first=s[40]))
    # the repeated key really is 2^64 - 1
    for n in (61, 253, 600):
        s = [TOP - 3 * (n - i) for i in range(n - 1)] + [TOP]
        d = s[:-2] + [TOP, TOP]
        name = "dup_pad_key_n%d" % n
        out.append(case(name, "dup", [permuted(d, affine(n))], dict(n=n, pair=(n - 2, n - 1), dup_key=TOP),
                        want=CRDT_E_DUP_KEY, twin=name + "_twin"))
        out.append(case(name + "_twin", "dup_twin", [permuted(s, affine(n))], dict(n=n)))
    # the negative control: a valid 2^64 - 1 as the last live key, pads after it
    for n in (63, 127, 255):
        s = [TOP - 3 * (n - 1 - i) for i in range(n)]
        out.append(case("top_then_pads_n%d" % n, "dup_twin", [permuted(s, affine(n))],
                        dict(n=n, epl=epl_of(n), widths=[32], pads=1)))
    return out


# ------------------------------------------------------------------ 6. layout

def layout_cases():
    out = []
    for R in (1, 3, 64):
        big0 = permuted([7 + 5 * i for i in range(300)], affine(300))
        big1 = permuted([9 + 5 * i for i in range(263)], reversal(263))
        small = permuted([100 + i for i in range(5)], reversal(5))
        docs = [big0, small, [], permuted([10 + 3 * i for i in range(70)], affine(70)), big1]
        out.append(case("layout_R%d" % R, "layout", docs, dict(at=0, n=300, path="block"), R=R, slack=(0, 1, 9, 9, 1)))
    return out


# ------------------------------------------------------------------ 7. counts above the slots

def over_case(name, n, claims, above=OVER):
    """[small, the bad document, a document with 14 entries and 12 spare slots, small]: an unclamped
    kernel reads `above` slots of the third document as the second's, and writes that many output
    slots of its region: all inside the arrays."""
    small = [30, 10, 20]
    bad = permuted([1000 + 3 * i for i in range(n)], affine(n))
    spare = permuted([5000 + 2 * i for i in range(14)], reversal(14))
    return case(name, "over", [small, bad, spare, small], dict(claims, at=1, n=n), slack=(2, 0, 12, 1), want=CRDT_E_CAPACITY,
                over=(1, above))


def over_cases():
    return [over_case("over_wave", 12, dict(path="wave", unclamped_path="wave")),
            over_case("over_block", 300, dict(path="block", unclamped_path="block")),
            # only the unclamped count crosses 256: the clamped size keeps the document on the wave path
            over_case("over_250_claims_259", 250, dict(path="wave", unclamped_path="block"))]


def all_cases() -> List[Case]:
    cases = (width_cases() + range_end_cases() + size_cases() + block_cases() + dup_cases() + layout_cases() + over_cases())
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}
CLEAN = [c for c in CASES if c.want is None]
DUP_CASES = [c for c in CASES if c.want == CRDT_E_DUP_KEY]
OVER_CASES = [c for c in CASES if c.over is not None]


def clean_of(R):
    return [c for c in CLEAN if c.R == R]


# ------------------------------------------------------------------ 8. the order check

ORDER_R = 3
ORDER_SIZES = (0, 1, 2, 64, 65, 66, 130)
LEAD = [5000 + 10 * i for i in range(3)]  # above every key of the document after it: a descent from document to document
TAIL = [1, 2, 3]


def sorted_doc(keys, d):
    return entries(keys, ORDER_R), clock(d, ORDER_R)


def order_positions(m):
    """The second index of every listed pair that exists in a document of m entries."""
    pos = {}
    if m >= 2:
        pos["first"] = 1
        pos["last"] = m - 1
    if m >= 65:
        pos["63_64"] = 64
    if m >= 66:
        pos["64_65"] = 65
    return pos


def order_case(name, keys, counted, want, claims, rows=None, srcs=None):
    docs = [sorted_doc(LEAD, 0), sorted_doc(keys, 1), sorted_doc(TAIL, 2)]
    rows = rows if rows is not None else [[], [], []]
    return OrderCase(name, ORDER_R, docs, rows, counted, srcs, dict(claims, at=1), want)


def garbage(n):
    """n slack entries with descending keys, the first below every live key of the table."""
    return entries([4 - (i % 4) for i in range(n)], ORDER_R)[:n] if n else []


def order_cases():
    out = []
    for m in ORDER_SIZES:
        keys = [10 + 10 * j for j in range(m)]
        for counted in (True, False):
            tag = "counts" if counted else "no_counts"
            out.append(order_case("order_clean_m%d_%s" % (m, tag), keys, counted, 0, dict(m=m, pair=None)))
            for pname, i in order_positions(m).items():
                inv = list(keys)
                inv[i - 1], inv[i] = inv[i], inv[i - 1]
                eq = list(keys)
                eq[i] = eq[i - 1]
                for kind, ks in (("inversion", inv), ("equal", eq)):
                    out.append(order_case("order_%s_m%d_%s_%s" % (kind, m, pname, tag), ks, counted, CRDT_E_UNSORTED,
                                          dict(m=m, pair=(i - 1, i), lane=(i - 1) % ORDER_LANES, kind=kind, counted=counted)))
    for counted in (True, False):
        tag = "counts" if counted else "no_counts"
        out.append(order_case("order_top_then_zero_%s" % tag, [10, 20, TOP, 0], counted, CRDT_E_UNSORTED,
                              dict(m=4, pair=(2, 3), lane=2)))
        out.append(order_case("order_zero_to_top_%s" % tag, [0, 20, TOP], counted, 0, dict(m=3, pair=None)))
    # 0 and 1 live entries over slots that hold descending keys; the three descents that are no violation
    for m in (0, 1):
        out.append(order_case("order_m%d_over_garbage" % m, [10][:m], True, 0, dict(m=m, pair=None),
                              rows=[garbage(2), garbage(70), garbage(1)]))
    keys = [10 + 10 * j for j in range(66)]
    out.append(order_case("order_descent_inside_slack", keys, True, 0, dict(m=66, pair=None),
                          rows=[[], entries([900, 800, 800, 700], ORDER_R), []]))
    out.append(order_case("order_descent_live_to_slack", keys, True, 0, dict(m=66, pair=None),
                          rows=[entries([4000], ORDER_R), entries([5], ORDER_R), entries([2], ORDER_R)]))
    out.append(order_case("order_descent_doc_to_doc", keys, False, 0, dict(m=66, pair=None, lead_last=LEAD[-1], first=10)))
    # fold forms: dst clean; a violation only in a source's entries, only in its tombstones; documents
    # with no source and a source with no entries ahead of the bad tombstone list
    good_e, good_t = entries([15, 25, 35], ORDER_R), entries([12, 22], ORDER_R)
    bad_e, bad_t = entries([15, 35, 25], ORDER_R), entries([22, 22], ORDER_R)
    vv = clock(5, ORDER_R)
    forms = {"clean": ([[(0, vv, good_e, good_t)], [(1, vv, good_e, good_t), (2, vv, good_e, [])], []], 0),
             "bad_entries": ([[(0, vv, good_e, good_t)], [(1, vv, good_e, good_t), (2, vv, bad_e, good_t)], []], CRDT_E_UNSORTED),
             "bad_tombs": ([[(0, vv, good_e, good_t)], [(1, vv, good_e, good_t)], [(2, vv, good_e, bad_t)]], CRDT_E_UNSORTED),
             "no_sources_then_bad_tombs": ([[], [], [(2, vv, [], bad_t)]], CRDT_E_UNSORTED),
             "no_sources": ([[], [], []], 0)}
    for name, (srcs, want) in forms.items():
        out.append(order_case("order_fold_%s" % name, keys, True, want, dict(m=66, pair=None, fold=name), srcs=srcs))
    assert len({c.name for c in out}) == len(out)
    return out


ORDER_CASES = order_cases()
ORDER_BY_NAME = {c.name: c for c in ORDER_CASES}


def order_batch(c: OrderCase):
    return pack(c.docs, c.R, [len(r) for r in c.slack_rows], rows=c.slack_rows, counted=c.counted)


def order_other(c: OrderCase):
    """A clean batch of as many documents, the other side of the case's join."""
    return pack([sorted_doc([15 + 20 * j for j in range(2 + d)], 7 + d) for d in range(len(c.docs))], c.R,
                [0] * len(c.docs))


def order_srcs(c: OrderCase):
    return SrcBatch.from_lists(c.R, c.srcs) if c.srcs is not None else None
