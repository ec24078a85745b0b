"""Deterministic join cases that sit on every edge of the plain join and exchange:
join_wave_kernel and join_block_kernel (csrc/join.hip), the tile kernels (csrc/tile.hip) and
block_merge (csrc/merge_block.hpp).

The wave kernel gives lane i the i-th entry of both sides of a document of at most 64 entries
a side, decides each with HasDot against the other side's clock, places the survivors with two
ballots and writes them in two halves of 64 slots, the staged stores padded to the end of a
64-byte sector (8 keys or counters, 16 actors) within the document's capacity.  A document
above 64 on either side is handed to the worklist: the tile kernels cut it into tiles of T
merged positions (a common key's pair may be cut apart), place each tile's survivors by a
look-back over the tiles before it, and the block kernel takes it whole.  Each Case below is
a handful of documents built by hand to put one of those quantities on a boundary; `claims`
names the edge in quantities `census` recomputes from the case and the oracle's result, so
that tests/test_join_edges_model.py fails when a case drifts off its edge; `want` is the first
document's result stated by hand, (dst <- src, src <- dst), where a case is about one outcome.

No RNG, no GPU.  Every case is R = 3.  A document is (entries [(key, actor, counter)], clock).
"""

from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np

from crdtgpu.batch import AWSetBatch
from join_option_cases import T_OF_SHAPE, WAVE_MAX
from test_tile_split_model import merge_path_in

U32, U64 = np.uint32, np.uint64
R = 3
TOP = (1 << 64) - 1
T_SMALL = T_OF_SHAPE[10]   # 512: the smallest tile shape
T_DEFAULT = T_OF_SHAPE[9]  # 1024: the default shape ("join_tile_shape" 9)
TILE_TS = (T_SMALL, T_DEFAULT)
WAVES, K_DEFAULT = 4, 8    # join.hip: kJoinWaves, the default "join_docs_per_wave"
OVER = 9                   # an over-count document claims this many entries above its slots (or as the case says)

FILLS = ("zeros", "ones", "continuation")
SLACKS = ((1, 9), (9, 1))  # (dst, src) slots added to every document by the slack-poison builds

Doc = Tuple[List[Tuple[int, int, int]], List[int]]


class Case(NamedTuple):
    name: str
    R: int
    dst_docs: List[Doc]
    src_docs: List[Doc]
    claims: Dict[str, object]          # census quantities of document claims["at"] (default 0)
    want: Optional[tuple] = None       # (entries of dst <- src, entries of src <- dst) of document 0, by hand
    slack: Optional[tuple] = None      # (per-document dst slack, per-document src slack); None: tight, no counts
    over: Optional[tuple] = None       # ("dst" | "src", document, n): its count is its slots + n
    shape: Optional[int] = None        # the join_tile_shape the case's sizes were built around


# ------------------------------------------------------------------ batches

def _continuation(ents, other_ents, other_vv, n):
    """n slack entries that would pass for live ones: keys ascending past the last live key,
    first the keys the other side holds live above it, under dots the other side's clock has
    not seen (one above its counter).  At the top of the key range the key repeats."""
    last = ents[-1][0] if ents else -1
    keys = [k for k, _, _ in other_ents if k > last][:n]
    nxt = (keys[-1] if keys else last) + 1
    while len(keys) < n:
        keys.append(min(nxt, TOP))
        nxt += 1
    return [(k, i % R, other_vv[i % R] + 1 + i) for i, k in enumerate(keys)]


def pack(docs, slacks, fill="zeros", others=None, over=None):
    """An AWSetBatch of docs with slacks[d] spare slots after document d, filled by `fill`;
    over = (document, count): that document's count as given.  counts is None where no
    document has slack and none is over."""
    n = len(docs)
    live = np.array([len(e) for e, _ in docs], dtype=np.int64)
    caps = live + np.array(slacks, dtype=np.int64)
    offsets = np.zeros(n + 1, dtype=U32)
    np.cumsum(caps, out=offsets[1:])
    total = int(offsets[-1])
    keys, actors, counters = np.zeros(total, U64), np.zeros(total, U32), np.zeros(total, U64)
    vv = np.zeros(n * R, U64)
    for d, (ents, v) in enumerate(docs):
        o = int(offsets[d])
        rows = list(ents)
        if fill == "ones":
            rows += [(TOP, 0xFFFFFFFF, TOP)] * slacks[d]
        elif fill == "continuation":
            rows += _continuation(ents, others[d][0], others[d][1], slacks[d])
        for i, (k, a, c) in enumerate(rows):
            keys[o + i], actors[o + i], counters[o + i] = k, a, c
        vv[d * R:(d + 1) * R] = v
    counts = live.astype(U32)
    if over is not None:
        counts[over[0]] = over[1]
    counted = over is not None or any(slacks)
    return AWSetBatch(R, offsets, keys, actors, counters, vv, counts if counted else None)


def slacks_of(case: Case, extra=(0, 0)):
    n = len(case.dst_docs)
    sd, ss = case.slack if case.slack else ([0] * n, [0] * n)
    return [x + extra[0] for x in sd], [x + extra[1] for x in ss]


def over_count(case: Case, extra=(0, 0)):
    """(side, document, unclamped count) of an over-count case."""
    side, d, above = case.over
    sl = slacks_of(case, extra)[0 if side == "dst" else 1]
    docs = case.dst_docs if side == "dst" else case.src_docs
    return side, d, len(docs[d][0]) + sl[d] + above


def batches(case: Case, extra=(0, 0), fill="zeros", clamped=False):
    """(a, b) host batches of a case.  An over-count case: with the bad count as the kernel
    gets it, or (clamped) with that count at the document's slots -- the batch the expectation
    is the oracle's join of."""
    sd, ss = slacks_of(case, extra)
    ov = {"dst": None, "src": None}
    if case.over:
        assert extra == (0, 0), "an over-count case keeps its own layout: its bad document has no slack"
        side, d, cnt = over_count(case, extra)
        ov[side] = (d, cnt - case.over[2] if clamped else cnt)
    a = pack(case.dst_docs, sd, fill, case.src_docs, ov["dst"])
    b = pack(case.src_docs, ss, fill, case.dst_docs, ov["src"])
    return a, b


def concat(cases, extra=(0, 0), fill="zeros"):
    """One batch pair of the documents of all `cases` in order, and the first document of each."""
    dd, sd, sld, sls, first = [], [], [], [], []
    for c in cases:
        assert c.over is None
        first.append(len(dd))
        a, b = slacks_of(c, extra)
        dd += c.dst_docs
        sd += c.src_docs
        sld += a
        sls += b
    return pack(dd, sld, fill, sd), pack(sd, sls, fill, dd), first


# ------------------------------------------------------------------ 1. the decide table

# name: (side of the deciding key, its dst dot, its src dot, dst clock, src clock, outcome in dst <- src,
#        outcome in src <- dst); an outcome is the dot the key is kept under, or None: removed.  One-sided keys
#        decide alike both ways: a dst-only key survives iff src's clock has not seen its dot, in either direction.
DECIDE = {
    # dst-only key against src's clock [5, 5, 5] at actor 1
    "dst_below_clock":  ("dst", (1, 4), None, [9, 9, 9], [0, 5, 0], None, None),
    "dst_at_clock":     ("dst", (1, 5), None, [9, 9, 9], [0, 5, 0], None, None),
    "dst_clock_plus_1": ("dst", (1, 6), None, [9, 9, 9], [0, 5, 0], (1, 6), (1, 6)),
    "dst_zero_at_zero": ("dst", (1, 0), None, [9, 9, 9], [7, 0, 7], None, None),
    "dst_actor_last":   ("dst", (R - 1, 5), None, [9, 9, 9], [0, 0, 5], None, None),   # kept if clock word 0 or 1 were read
    "dst_actor_above":  ("dst", (R + 1, 1), None, [9, 9, 9], [9, 9, 9], (R + 1, 1), (R + 1, 1)),  # never seen
    # the mirror: src-only key against dst's clock
    "src_below_clock":  ("src", None, (1, 4), [0, 5, 0], [9, 9, 9], None, None),
    "src_at_clock":     ("src", None, (1, 5), [0, 5, 0], [9, 9, 9], None, None),
    "src_clock_plus_1": ("src", None, (1, 6), [0, 5, 0], [9, 9, 9], (1, 6), (1, 6)),
    "src_zero_at_zero": ("src", None, (1, 0), [7, 0, 7], [9, 9, 9], None, None),
    "src_actor_last":   ("src", None, (R - 1, 5), [0, 0, 5], [9, 9, 9], None, None),
    "src_actor_above":  ("src", None, (R + 1, 1), [9, 9, 9], [9, 9, 9], (R + 1, 1), (R + 1, 1)),
    # common key: kept whatever the clocks say; the src dot wins, so each direction ends with the other's dot
    "common_same_dot":  ("both", (1, 3), (1, 3), [1, 1, 1], [1, 1, 1], (1, 3), (1, 3)),
    "common_src_wins":  ("both", (0, 2), (1, 7), [2, 0, 0], [0, 7, 0], (1, 7), (0, 2)),
    "common_covered":   ("both", (0, 2), (1, 3), [2, 9, 0], [9, 3, 0], (1, 3), (0, 2)),
}
COMMON_KINDS = ("common_same_dot", "common_src_wins", "common_covered")
# position of the deciding entry in its own side: (entries of that side, index)
POSITIONS = {"lane0": (3, 0), "last": (3, 2), "lane63": (64, 63), "block": (66, 65)}
FILLER_DOT = (0, 1)  # every other key is common under this dot: kept both ways whatever the clocks


def decide_docs(kind, n, p):
    """The document pair of a decide case: n - 1 common filler keys 10, 20, ... and the
    deciding key 10 p + 5 at index p of its side; and the hand-stated results."""
    side, ddot, sdot, dvv, svv, out_ab, out_ba = DECIDE[kind]
    fillers = [(10 * (j + 1),) + FILLER_DOT for j in range(n - 1)]
    key = 10 * p + 5
    dst = sorted(fillers + ([(key,) + ddot] if ddot else []))
    src = sorted(fillers + ([(key,) + sdot] if sdot else []))
    want = tuple(sorted(fillers + ([(key,) + out] if out else [])) for out in (out_ab, out_ba))
    return (dst, dvv), (src, svv), want, key


def decide_cases():
    out = []
    for kind in DECIDE:
        for pos, (n, p) in POSITIONS.items():
            d, s, want, key = decide_docs(kind, n, p)
            out.append(Case("decide_%s_%s" % (kind, pos), R, [d], [s],
                            dict(key=key, lane=p, n_out=len(want[0]), path="wave" if n <= WAVE_MAX else "large"),
                            want=want))
    return out


# ------------------------------------------------------------------ 2. wave shapes

VV = [5, 5, 5]


def one_sided(keys, shift=0):
    """Entries under the clock VV of the other side: every third is covered (removed), the
    others are one above the clock (kept)."""
    return [(k, (i + shift) % R, 5 if (i + shift) % 3 == 0 else 6) for i, k in enumerate(keys)]


def kept(keys, actor=0):
    return [(k, (actor + i) % R, 6 + i % 3) for i, k in enumerate(keys)]


def removed(keys):
    return [(k, i % R, 5 - i % 2) for i, k in enumerate(keys)]


LAYOUTS = ("common", "dst_below", "src_below", "interleaved")


def layout_docs(dn, sn, layout):
    """(dst, src) documents of dn and sn entries; common: the first min(dn, sn) keys shared under
    different dots, the longer side's rest after them."""
    if layout == "common":
        m = min(dn, sn)
        shared = [100 + 2 * i for i in range(m)]
        dk = shared + [1000 + 2 * i for i in range(dn - m)]
        sk = shared + [1001 + 2 * i for i in range(sn - m)]
        dst = [(k, 0, 1 + i % 4) for i, k in enumerate(shared)] + one_sided(dk[m:])
        src = [(k, 1, 2 + i % 4) for i, k in enumerate(shared)] + one_sided(sk[m:], 1)
        return (dst, VV), (src, VV)
    if layout == "dst_below":
        dk, sk = [10 + i for i in range(dn)], [500 + i for i in range(sn)]
    elif layout == "src_below":
        dk, sk = [500 + i for i in range(dn)], [10 + i for i in range(sn)]
    else:  # strictly interleaved: dst even, src odd
        dk, sk = [10 + 2 * i for i in range(dn)], [11 + 2 * i for i in range(sn)]
    return (one_sided(dk), VV), (one_sided(sk, 1), VV)


WAVE_SIZES = (0, 1, 63, 64)
SMALL_D: Doc = ([(3, 0, 6), (7, 1, 2), (9, 2, 6)], [1, 2, 3])
SMALL_S: Doc = ([(5, 1, 4), (7, 2, 1), (11, 0, 1)], [2, 2, 2])  # join: 3 (0 6), 5 (1 4), 7 (2 1), 9 (2 6)


def wave_shape_cases():
    out = []
    for dn in WAVE_SIZES:
        for sn in WAVE_SIZES:
            for layout in LAYOUTS:
                d, s = layout_docs(dn, sn, layout)
                out.append(Case("wave_%d_%d_%s" % (dn, sn, layout), R, [d, SMALL_D], [s, SMALL_S],
                                dict(dn=dn, sn=sn, layout=layout, path="wave")))
    return out


# n_out: (dst kept, dst removed, src kept, src removed), strictly interleaved
N_OUT = {0: (0, 64, 0, 64), 1: (1, 63, 0, 64), 63: (32, 32, 31, 33), 64: (32, 0, 32, 0), 65: (64, 0, 1, 63),
         127: (64, 0, 63, 1), 128: (64, 0, 64, 0)}


def mixed_doc(n_kept, n_removed, key0, step=2):
    """n_kept + n_removed one-sided entries from key0 up, the removed ones spread among the kept."""
    n = n_kept + n_removed
    ents, k, r = [], 0, 0
    for i in range(n):
        keep = k < n_kept and (r >= n_removed or (i * n_kept) // n >= k)
        key = key0 + step * i
        if keep:
            ents.append((key, i % R, 6 + i % 3))
            k += 1
        else:
            ents.append((key, i % R, 5 - i % 2))
            r += 1
    assert k == n_kept and r == n_removed
    return ents


def n_out_cases():
    out = []
    for n_out, (dk, dr, sk, sr) in N_OUT.items():
        d, s = (mixed_doc(dk, dr, 10), VV), (mixed_doc(sk, sr, 11), VV)
        out.append(Case("n_out_%d" % n_out, R, [d, SMALL_D], [s, SMALL_S], dict(n_out=n_out, path="wave")))
    return out


END_MOD16 = (0, 1, 7, 8, 9, 15)  # (obase + n_out) mod 16; mod 8 these are 0, 1, 7, 0, 1, 7
PAD_N = (20, 17)                 # the padded document: 37 survivors, everything kept


def pad_cases():
    """[lead, the document, tail]: the lead's size puts the end of the document's survivors on
    each residue; with an output capacity of exactly n_out (the next document starts at the
    next slot) and with five spare slots."""
    out = []
    n_out = sum(PAD_N)
    for res in END_MOD16:
        for exact in (True, False):
            p = (res - n_out) % 16 + 16
            lead = (kept([10 + i for i in range(p)]), VV)
            d = (kept([10 + 2 * i for i in range(PAD_N[0])]), VV)
            s = (kept([11 + 2 * i for i in range(PAD_N[1])], 1), VV)
            slack = None if exact else ([0, 5, 0], [0, 0, 0])
            out.append(Case("pad_end_%d_%s" % (res, "exact" if exact else "spare"), R, [lead, d, SMALL_D],
                            [([], VV), s, SMALL_S],
                            dict(at=1, n_out=n_out, end_mod16=res, end_mod8=res % 8, cap_exact=exact, path="wave"),
                            slack=slack))
    return out


def empty_between_case():
    full_d, full_s = (kept([10 + 2 * i for i in range(64)]), VV), (kept([11 + 2 * i for i in range(64)], 1), VV)
    gone_d, gone_s = (removed([10 + 2 * i for i in range(64)]), VV), (removed([11 + 2 * i for i in range(64)]), VV)
    return [Case("no_survivors_between_two_full", R, [full_d, gone_d, full_d], [full_s, gone_s, full_s],
                 dict(at=1, n_out=0, path="wave", n_out_before=128, n_out_after=128))]


# ------------------------------------------------------------------ 3. handoff to the worklist

HANDOFF_SIZES = ((64, 65), (65, 64), (65, 0), (0, 65))
LAST_OF_K = WAVES * (K_DEFAULT - 1)  # document 28: wave 0's last (k = 7) at the default K


def handoff_cases():
    out = []
    for dn, sn in HANDOFF_SIZES:
        d, s = layout_docs(dn, sn, "interleaved")
        for place, n_docs, at in (("first", 5, 0), ("last", 5, 4), ("last_of_k", LAST_OF_K + 5, LAST_OF_K)):
            dd, sd = [SMALL_D] * n_docs, [SMALL_S] * n_docs
            dd[at], sd[at] = d, s
            out.append(Case("handoff_%d_%d_%s" % (dn, sn, place), R, dd, sd,
                            dict(at=at, dn=dn, sn=sn, path="large", place=place, k_slot=(at % (WAVES * K_DEFAULT)) // WAVES)))
    return out


# ------------------------------------------------------------------ 4. block and tile

def alternating(total, outcome=one_sided):
    """total merged positions, dst at the even ones and src at the odd ones."""
    dk = [10 * (i + 1) for i in range(0, total, 2)]
    sk = [10 * (i + 1) for i in range(1, total, 2)]
    return outcome(dk), outcome(sk)


def by_position(total, keep):
    """total alternating one-sided entries, merged position i kept iff keep(i)."""
    dst, src = [], []
    for i in range(total):
        e = (10 * (i + 1), i % R, 6 if keep(i) else 5)
        (dst if i % 2 == 0 else src).append(e)
    return dst, src


def straddle_docs(T, kind):
    """Merged positions 0 .. T - 2 one-sided and alternating, then a common key whose dst half
    is position T - 1 (the last of tile 0) and whose src half is position T (the first of tile
    1), then 40 more.  The pair's dots and the clocks' words they meet are the decide table's;
    the one-sided entries sit at actor 2, whose clock word (5) the table's rows leave alone."""
    _, ddot, sdot, dvv, svv, out_ab, out_ba = DECIDE[kind]
    dvv, svv = dvv[:2] + [5], svv[:2] + [5]
    dst, src = [], []
    for i in list(range(T - 1)) + list(range(T + 1, T + 41)):
        e = (10 * (i + 1), 2, 5 if i % 3 == 0 else 6)
        (dst if i % 2 == 0 else src).append(e)
    key = 10 * T + 5
    dst = sorted(dst + [(key,) + ddot])
    src = sorted(src + [(key,) + sdot])
    return (dst, dvv), (src, svv), key, (out_ab, out_ba)


def tile_cases():
    out = []
    for T in TILE_TS:
        shape = 10 if T == T_SMALL else 9
        tag = "T%d" % T
        for total in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
            d, s = alternating(total)
            out.append(Case("tile_%s_total_%d" % (tag, total), R, [(d, VV)], [(s, VV)],
                            dict(total=total, T=T, tiles=-(-total // T), path="large"), shape=shape))
        for kind in COMMON_KINDS:
            d, s, key, outs = straddle_docs(T, kind)
            out.append(Case("tile_%s_straddle_%s" % (tag, kind), R, [d], [s],
                            dict(T=T, straddle_key=key, dot_ab=outs[0], dot_ba=outs[1], path="large"), shape=shape))
        first = by_position(T + 40, lambda i: i >= T)
        middle = by_position(2 * T + 40, lambda i: not T <= i < 2 * T)
        none = by_position(T + 40, lambda i: False)
        every = by_position(T + 40, lambda i: True)
        for name, (d, s), claims in (
                ("first_tile_removed", first, dict(zero_tiles=[0], n_out=40)),
                ("middle_tile_removed", middle, dict(zero_tiles=[1], n_out=T + 40)),
                ("all_removed", none, dict(zero_tiles=[0, 1], n_out=0)),
                ("all_kept", every, dict(zero_tiles=[], n_out=T + 40))):
            out.append(Case("tile_%s_%s" % (tag, name), R, [(d, VV)], [(s, VV)], dict(claims, T=T, path="large"),
                            shape=shape))
        n = T // 2 + 20
        below = one_sided([10 + i for i in range(n)]), one_sided([100000 + i for i in range(n)], 1)
        out.append(Case("tile_%s_dst_below_src" % tag, R, [(below[0], VV)], [(below[1], VV)],
                        dict(T=T, one_side_below=True, path="large"), shape=shape))
    return out


# ------------------------------------------------------------------ 5. the key range

def key_range_cases():
    """Keys 0 and 2^64 - 1 (the merge path's own pad value) live on dst only, on src only and
    on both; dst is always the shorter run, so 2^64 - 1 ends the shorter run, the longer one,
    or both."""
    out = []
    for path, (nd, ns), shape in (("wave", (5, 8), None), ("large", (70, 80), None), ("tile", (200, T_SMALL + 1 - 200), 10)):
        for where in ("dst", "src", "both"):
            dk = [1000 + 3 * i for i in range(nd - 2)]
            sk = [1001 + 3 * i for i in range(ns - 2)]
            ends = [0, TOP]
            dk = sorted(dk + (ends if where in ("dst", "both") else [500, 900000]))
            sk = sorted(sk + (ends if where in ("src", "both") else [501, 900001]))
            d = [(k, i % R, 6 + i % 2) for i, k in enumerate(dk)]  # everything kept: 0 and TOP are in the result
            s = [(k, (i + 1) % R, 6 + i % 3) for i, k in enumerate(sk)]
            out.append(Case("keys_0_top_%s_%s" % (where, path), R, [(d, VV), SMALL_D], [(s, VV), SMALL_S],
                            dict(ends_in=where, top_ends={"dst": "shorter", "src": "longer", "both": "both"}[where],
                                 path="wave" if path == "wave" else "large", tiles_small=2 if path == "tile" else None),
                            shape=shape))
    return out


# ------------------------------------------------------------------ 6. counts above the slots

def spare_doc(key0, n=14):
    return (kept([key0 + 2 * i for i in range(n)]), VV)


def over_case(name, side, nd, ns, claims, shape=None, above=OVER):
    """[small, the bad document, a document with 14 entries and 12 spare slots a side, small]:
    an unclamped kernel reads OVER entries of the third document as the second's and writes at
    most that many slots into its output region, all inside the arrays."""
    d, s = alternating(nd + ns) if nd == ns else (one_sided([10 + 2 * i for i in range(nd)]),
                                                  one_sided([11 + 2 * i for i in range(ns)], 1))
    assert len(d) == nd and len(s) == ns
    dd = [SMALL_D, (d, VV), spare_doc(5000), SMALL_D]
    sd = [SMALL_S, (s, VV), spare_doc(5001), SMALL_S]
    return Case(name, R, dd, sd, dict(claims, at=1, dn=nd, sn=ns), slack=([2, 0, 12, 1], [1, 0, 12, 2]),
                over=(side, 1, above), shape=shape)


def over_cases():
    out = []
    tile_n = ((T_SMALL + 1) // 2, T_SMALL + 1 - (T_SMALL + 1) // 2)
    for side in ("dst", "src"):
        out.append(over_case("over_%s_wave" % side, side, 10, 12, dict(path="wave", unclamped_path="wave")))
        out.append(over_case("over_%s_block" % side, side, 80, 80, dict(path="large", unclamped_path="large")))
        out.append(over_case("over_%s_tile" % side, side, tile_n[0], tile_n[1],
                             dict(path="large", unclamped_path="large", total=T_SMALL + 1, tiles_small=2), shape=10))
    # only the unclamped count crosses 64: the clamped sizes keep the document on the wave path
    out.append(over_case("over_dst_60_claims_70", "dst", 60, 12, dict(path="wave", unclamped_path="large"), above=10))
    # the same against a large other side: the block and tile paths merge 60 entries, not 70
    out.append(over_case("over_dst_60_claims_70_against_80", "dst", 60, 80, dict(path="large", unclamped_path="large"),
                         above=10))
    return out


def all_cases() -> List[Case]:
    cases = (decide_cases() + wave_shape_cases() + n_out_cases() + pad_cases() + empty_between_case() + handoff_cases() +
             tile_cases() + key_range_cases() + over_cases())
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}
TABLE = [c for c in CASES if c.over is None]   # the cases that run clean
OVER_CASES = [c for c in CASES if c.over is not None]


# ------------------------------------------------------------------ census

def path_of(nd, ns):
    """The kernel a document's (clamped) sizes select: the wave kernel merges it, or hands it
    to the worklist (the tile kernels, or join_block_kernel)."""
    return "wave" if nd <= WAVE_MAX and ns <= WAVE_MAX else "large"


def tile_census(dst, src, result_keys, T):
    """Per tile of T merged positions (dst first on equal keys): survivors placed by the tile
    (a common key counts at its dst half), and the merge-path split at each tile's diagonal."""
    dk, sk = [k for k, _, _ in dst], [k for k, _, _ in src]
    nd, ns = len(dk), len(sk)
    total = nd + ns
    n_tiles = max(1, -(-total // T))
    splits = []
    for t in range(n_tiles + 1):
        k = min(t * T, total)
        i = merge_path_in(dk, sk, k, max(0, k - ns), min(k, nd))
        splits.append((i, k - i))
    res, dset = set(result_keys), set(dk)
    survivors = []
    for t in range(n_tiles):
        (i0, j0), (i1, j1) = splits[t], splits[t + 1]
        n = sum(1 for k in dk[i0:i1] if k in res) + sum(1 for k in sk[j0:j1] if k in res and k not in dset)
        survivors.append(n)
    assert sum(survivors) == len(res)
    return dict(n_tiles=n_tiles, splits=splits, survivors=survivors)


def census(case: Case, result):
    """Quantities of document claims["at"] recomputed from the case and `result`, the oracle's
    entries of dst <- src for that document: sizes, path, n_out, where the output ends, the
    lane of the deciding key, and per tile size the tiles' survivors and splits."""
    at = case.claims.get("at", 0)
    dst, src = case.dst_docs[at][0], case.src_docs[at][0]
    sd, ss = slacks_of(case)
    obase = sum(len(e) for e, _ in case.dst_docs[:at]) + sum(sd[:at]) + sum(len(e) for e, _ in case.src_docs[:at]) + sum(ss[:at])
    n_out = len(result)
    cap = len(dst) + sd[at] + len(src) + ss[at]
    out = dict(at=at, dn=len(dst), sn=len(src), path=path_of(len(dst), len(src)), n_out=n_out, obase=obase,
               end_mod8=(obase + n_out) % 8, end_mod16=(obase + n_out) % 16, cap_exact=cap == n_out,
               k_slot=(at % (WAVES * K_DEFAULT)) // WAVES, total=len(dst) + len(src))
    rk = [k for k, _, _ in result]
    out["tiles"] = {T: tile_census(dst, src, rk, T) for T in TILE_TS}
    if case.over:
        side, d, cnt = over_count(case)
        nd, ns = (cnt, len(src)) if side == "dst" else (len(dst), cnt)
        out["unclamped_path"] = path_of(nd, ns)
    return out
