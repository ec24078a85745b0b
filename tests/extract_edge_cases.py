"""Deterministic extraction cases that sit on every edge of extract_kernel (csrc/extract.hip).

The kernel gives a wavefront a group of G = 64 / R consecutive documents (lane j*R + r holds
P[r] of the group's j-th document), stages the group's sources 128 at a time (kExSrcs),
streams the staged run's entries and tombstones 64 lanes at a time starting at the run's
first position (not at a multiple of 64), finds each lane's source by a search over the
staged offsets, and rebuilds the packed offset of an empty source from its neighbours
(mark_first walks back from the next non-empty source, a tail pass takes the empties at
the end of a run).  Each Case below is a few documents built by hand to put one of those
quantities on a boundary.  `census` computes from the layout alone which edges a case
reaches; tests/test_extract_edges_model.py asserts from it that every edge is reached by a
named case, so a later edit to the table cannot drop one unnoticed.

A case is (name, R, per_doc, peers): per_doc[d] lists the sources of document d as
(actor, vv, entries [(k, a, c)], tombstones [(k, a, c)] or None), the shape extract_ref of
tests/test_delta_extract_model.py takes, and peers[d] is the clock the peer has reached.
Expected results are that restatement's.
"""

from __future__ import annotations

from typing import List, NamedTuple, Optional

import test_delta_extract_model as model

TOP = (1 << 64) - 1
HALF = 1 << 63
BIG_ACTOR = 0xFFFFFFFF

# Restated from csrc/extract.hip, on purpose not imported from a build:
WAVE = 64   # lanes of a wavefront; launch_extract: G = 64u / sv.R documents a group
RUN = 128   # kExSrcs: sources a wavefront stages at a time (the loop over sb)
CHUNK = 64  # positions of one step of the entry and tombstone loops (base += 64)

GEOMETRY_R = (1, 2, 3, 5, 21, 22, 31, 32, 33, 63, 64)
RUN_SIZES = (127, 128, 129, 256, 257)
TOTALS = (0, 1, 63, 64, 65, 128, 129)


class Case(NamedTuple):
    name: str
    R: int
    per_doc: list
    peers: list
    kind_null: bool = False            # the call passes kind == NULL
    tombs: str = "given"               # "given"; srcs->tomb_off == NULL with the output's tombstone
    #                                    arrays "out_null" or its tomb_off "out_given"


def group_size(R):
    return WAVE // R


# ------------------------------------------------------------------ builders

def clock(R, d):
    """The peer clock of document d: 0 where d + r is even, so that every actor is unseen by
    one of two neighbouring documents and seen by the other, and the seen values differ."""
    return [0 if (d + r) % 2 == 0 else 10 + (d + 3 * r) % 7 for r in range(R)]


def seen(P):
    return [r for r, p in enumerate(P) if p]


def unseen(P):
    return [r for r, p in enumerate(P) if not p]


def vv_of(R, i):
    return [(i * 5 + r * 3) % 11 + 1 for r in range(R)]


def delta_src(P, keep, tombs=None, key0=1, step=2, i=0):
    """A DELTA source under P (its actor is the last one P has seen): entry j is kept iff
    keep[j].  Kept dots are one above the peer's counter, an actor the peer never met, or an
    actor above R; withheld dots are equal to the peer's counter or one below."""
    R, s, u = len(P), seen(P), unseen(P)
    assert s, "a DELTA source needs an actor the peer has seen"
    ents = []
    for j, kp in enumerate(keep):
        b = s[j % len(s)]
        if kp:
            dot = ((b, P[b] + 1), (u[j % len(u)], 3) if u else (b, P[b] + 2), (R + 1, 1))[j % 3]
        else:
            dot = (b, P[b] - (j % 2))
        ents.append((key0 + step * j,) + dot)
    return (s[-1], vv_of(R, i), ents, tombs)


def full_src(P, n, tombs=None, key0=1, step=2, i=0, actor=None):
    """A FULL source under P: its actor is one P never met (or above R); n entries, every
    other one with a dot P covers, which a DELTA would withhold."""
    R, s, u = len(P), seen(P), unseen(P)
    a = actor if actor is not None else (u[-1] if u else R + 1)
    ents = []
    for j in range(n):
        dot = (s[j % len(s)], P[s[j % len(s)]]) if s and j % 2 else ((u[0], 3) if u else (R + 1, 2))
        ents.append((key0 + step * j,) + dot)
    return (a, vv_of(R, i), ents, tombs)


def tombs_on(ents, keep, other):
    """One tombstone per entry key: kept (same actor, counter equal or above the entry's) or
    dropped (another actor `other`, or the entry's counter higher)."""
    out = []
    for j, ((k, a, c), kp) in enumerate(zip(ents, keep)):
        if kp:
            out.append((k, a, c + j % 2))
        elif j % 2 or c < 2:
            out.append((k, other if other != a else other + 1, c))
        else:
            out.append((k, a, c - 1))
    return out


def free_tombs(n, key0=2, step=2, actor=0):
    """n tombstones on keys no entry holds (even keys; the builders' entries are odd)."""
    return [(key0 + step * j, actor, 1 + j % 4) for j in range(n)]


# ------------------------------------------------------------------ 1. R and groups

def geo_doc(R, d):
    """Document d of a geometry case: a DELTA source at an actor its peer has seen and a FULL
    one at an actor it has not; the neighbouring documents' clocks turn both around, and
    cover the kept dots and uncover the withheld ones.  Every fifth document has no source."""
    P = clock(R, d)
    if d % 5 == 3:
        return []
    s, u = seen(P), unseen(P)
    k = 1000 * d + 1
    out = []
    if s:
        a, b = s[-1], s[0]
        ents = [(k, b, P[b]), (k + 2, a, P[a] + 1)] + ([(k + 4, u[-1], 3)] if u else [])
        out.append((a, vv_of(R, d), ents, [(k, b, P[b]), (k + 1, a, 1)]))
    if u:
        ents = [(k + 10, u[0], 3)] + ([(k + 12, s[-1], 2)] if s else [(k + 12, u[-1], 9)])
        out.append((u[-1], vv_of(R, d + 1), ents, [(k + 11, u[0], 2)]))
    return out


def doc_counts(R):
    G = group_size(R)
    return sorted({1, G - 1, G, G + 1, 2 * G} - {0}) if G > 1 else [1, 2, 3]


def geometry_cases():
    out = []
    for R in GEOMETRY_R:
        for n in doc_counts(R):
            out.append(Case("geo_R%d_docs%d" % (R, n), R, [geo_doc(R, d) for d in range(n)],
                            [clock(R, d) for d in range(n)]))
    return out


# ------------------------------------------------------------------ 2. staging runs

def small_src(P, i, pattern=None):
    """Source i of a run case, by pattern: 0 DELTA, an entry kept, one withheld, a tombstone;
    1 FULL, one entry; 2 DELTA, a tombstone and no entry; 3 DELTA, three entries all withheld
    (NONE: its input range is not empty, its packed range is); 4 empty; 5 FULL, two entries
    and two tombstones, one of them on a key added again."""
    pattern = i % 6 if pattern is None else pattern
    k = 40 * i + 1
    if pattern == 0:
        return delta_src(P, [True, False], free_tombs(1, k + 1), key0=k, i=i)
    if pattern == 1:
        return full_src(P, 1, [], key0=k, i=i)
    if pattern == 2:
        return delta_src(P, [], free_tombs(1, k + 1, actor=len(P) + 1), key0=k, i=i)
    if pattern == 3:
        return delta_src(P, [False] * 3, [], key0=k, i=i)
    if pattern == 4:
        return delta_src(P, [], [], key0=k, i=i)
    src = full_src(P, 2, None, key0=k, i=i)
    return src[:3] + (tombs_on(src[2], [True, False], other=len(P) + 1),)


def spread(n_srcs, n_docs):
    """n_srcs sources over n_docs documents: one, none, the bulk, then 0 / 1 / 2 in turn."""
    counts = [1, 0, 0] + [d % 3 for d in range(3, n_docs)]
    counts[2] = n_srcs - sum(counts)
    assert counts[2] > 0
    return counts


def run_case(name, n_srcs, patterns=None, R=2):
    """A light group, the group of n_srcs sources, and three trailing documents."""
    G = group_size(R)
    patterns = patterns or {}
    per_doc, peers = [], []
    for d in range(G):  # the light group: the heavy one's packed base is not 0
        peers.append(clock(R, d))
        per_doc.append([small_src(peers[-1], d)] if d % 2 else [])
    i = 0
    for d, n in enumerate(spread(n_srcs, G), start=G):
        peers.append(clock(R, d))
        per_doc.append([small_src(peers[-1], i + j, patterns.get(i + j)) for j in range(n)])
        i += n
    for d in range(2 * G, 2 * G + 3):
        peers.append(clock(R, d))
        per_doc.append([small_src(peers[-1], d + j) for j in range(d % 3 + 1)])
    return Case(name, R, per_doc, peers)


def staging_cases():
    out = [run_case("run_%d" % n, n) for n in RUN_SIZES]
    out += [
        run_case("seam_nonempty_both_sides", 130, {127: 0, 128: 0}),
        run_case("seam_empty_last_of_run0", 130, {127: 4, 128: 0}),
        run_case("seam_empty_first_of_run1", 130, {127: 0, 128: 4}),
        run_case("seam_empty_on_both_sides", 130, {126: 0, 127: 4, 128: 4, 129: 0}),
        run_case("run_of_128_empties", 261, {**{i: 4 for i in range(128, 256)}, 127: 0, 256: 0}),
        run_case("run_keeps_nothing", 140, {**{i: 3 for i in range(128)}, 128: 0}),
    ]
    R = 64
    P = [clock(R, d) for d in range(3)]
    out.append(Case("one_doc_130_sources_R64", R,
                    [[small_src(P[0], 0)], [small_src(P[1], i) for i in range(130)], [small_src(P[2], 5)]], P))
    return out


# ------------------------------------------------------------------ 3. empty sources inside a run

def empties_case(which, n):
    """[n empty, full, n empty, full, n empty] as all the sources of one group, between a group
    before and a group after; `which`: e = no entries (tombstones only), t = no tombstones
    (entries only), both."""
    R = 5
    G = group_size(R)
    P = [clock(R, d) for d in range(2 * G + 1)]

    def empty(i):
        if which == "e":
            return delta_src(P[G], [], free_tombs(2, 40 * i + 2), i=i)
        if which == "t":
            return delta_src(P[G], [True, False, True], [], key0=40 * i + 1, i=i)
        return delta_src(P[G], [], [], i=i)

    mid, i = [], 0
    for block in range(3):
        for _ in range(n):
            mid.append(empty(i))
            i += 1
        if block < 2:
            mid.append(small_src(P[G], i, 0 if block else 5))
            i += 1
    per_doc = [[] for _ in P]
    per_doc[0], per_doc[G], per_doc[2 * G] = [small_src(P[0], 0)], mid, [small_src(P[2 * G], 5)]
    return Case("empties_%s_%d" % (which, n), R, per_doc, P)


def empties_cases():
    out = [empties_case(w, n) for w in ("both", "e", "t") for n in (1, 2, 3)]
    R = 5
    P = [clock(R, d) for d in range(2)]
    nothing_kept = lambda i: small_src(P[1], i, 3)  # noqa: E731
    empty = lambda i: small_src(P[1], i, 4)  # noqa: E731
    out.append(Case("all_dropped_next_to_empty", R,
                    [[small_src(P[0], 9, 0)],
                     [small_src(P[1], 0, 0), nothing_kept(1), empty(2), small_src(P[1], 3, 0), empty(4), nothing_kept(5),
                      small_src(P[1], 6, 5), nothing_kept(7), empty(8)]], P))
    return out


# ------------------------------------------------------------------ 4. chunks

def split_sizes(n):
    """n elements in sources of 63, 1, 1 and the rest: starts at run positions 0, 63, 64, 65."""
    out = []
    for s in (63, 1, 1):
        if n > 0:
            out.append(min(s, n))
            n -= out[-1]
    return out + ([n] if n else []) or [0, 0]


def chunk_frame(R, mid):
    """A five-entry, three-tombstone document first, so that no run starts at a multiple of 64."""
    P = [clock(R, d) for d in range(3)]
    lead = delta_src(P[0], [True] * 5, free_tombs(3), i=7)
    return [[lead], mid(P[1]), [small_src(P[2], 3, 0)]], P


def total_case(which, n):
    R = 33  # G = 1: the run is the document's

    def mid(P):
        out, k = [], 1
        for i, s in enumerate(split_sizes(n)):
            if which == "e":
                out.append(delta_src(P, [(j + i) % 3 != 1 for j in range(s)], free_tombs(2, k + 1) if n == 0 else [], key0=k, i=i))
            else:  # s tombstones; from the second on each sits on an entry's key, every third added again
                src = full_src(P, s - 1 if s else 2, None, key0=k + 2, i=i)  # (no tombstone: two entries)
                tombs = [(k, 0, 1)][:s] + tombs_on(src[2], [j % 3 != 0 for j in range(s - 1)], other=R + 1)
                out.append(src[:3] + (tombs,))
            k += 2 * s + 10
        return out

    per_doc, P = chunk_frame(R, mid)
    return Case("%s_total_%d" % (which, n), R, per_doc, P)


def mask_keep():
    """Six chunks: full, empty, lane 0 only, lane 63 only, alternating, full."""
    rows = ([True] * 64, [False] * 64, [j == 0 for j in range(64)], [j == 63 for j in range(64)],
            [j % 2 == 0 for j in range(64)], [True] * 64)
    return [x for r in rows for x in r]


def mask_cases():
    R = 33
    keep = mask_keep()

    def e_mid(P):
        return [delta_src(P, keep, [], i=1)]

    def t_mid(P):
        src = full_src(P, len(keep), None, i=1)
        return [src[:3] + (tombs_on(src[2], keep, other=R + 1),)]

    out = []
    for name, mid in (("e_masks", e_mid), ("t_masks", t_mid)):
        per_doc, P = chunk_frame(R, mid)
        out.append(Case(name, R, per_doc, P))
    return out


def chunk_cases():
    return [total_case(w, n) for w in ("e", "t") for n in TOTALS] + mask_cases()


# ------------------------------------------------------------------ 5. the re-add filter

def readd_cases():
    R = 3
    P = [[4, 4, 4], [4, 0, 4], [4, 4, 0]]
    ents = [(10, 0, 5), (20, 1, 5), (30, 2, 5), (40, 0, 5)]
    positions = [
        (0, [1, 1, 1], ents, [(5, 0, 1), (50, 0, 1)]),                  # below every entry key, above every one
        (0, [1, 1, 1], ents, [(10, 0, 4), (40, 0, 4)]),                 # the first and the last key: added again
        (0, [1, 1, 1], ents, [(10, 0, 5), (40, 0, 6)]),                 # the same with counter equal, entry's lower: kept
        (0, [1, 1, 1], ents, [(10, 1, 9), (20, 1, 5), (30, 0, 9)]),     # another actor: dropped whatever the counter
        (1, [1, 1, 1], [], [(0, 0, 1), (7, 1, 2), (TOP, 2, 3)]),        # no entries: the search runs over nothing
    ]
    wide = [
        (0, [2, 2, 2], [(0, 0, 3), (HALF, 1, 3), (TOP, 2, 3)], [(0, 0, 2), (HALF, 1, 3), (TOP, 0, 1)]),
        (1, [2, 2, 2], [(HALF, 1, 3)], [(0, 0, 2), (HALF - 1, 1, 3), (HALF + 1, 1, 3), (TOP, 0, 1)]),
        (2, [2, 2, 2], [(0, 0, 3), (TOP, 2, 3)], [(HALF, 0, 2)]),
    ]
    beyond = [  # tombstone dots at actor R and above: never tested, shipped unless the key was added again
        (0, [3, 3, 3], [(10, 0, 5), (20, R + 1, 5)], [(5, R, 1), (10, R, 9), (15, R + 1, 1), (20, R + 1, 5), (25, BIG_ACTOR, TOP)]),
    ]
    out = [Case("readd_positions", R, [positions, wide, beyond], P)]
    for nt in (64, 65):
        for ne in (1, 130):
            ents = [(6 * j, j % R, 2 + j % 3) for j in range(ne)] if ne > 1 else [(30, 1, 2)]
            emap = {k: (a, c) for k, a, c in ents}
            tombs = []
            for j in range(nt):
                k = 3 * j
                if k in emap:  # a hit: other actor, equal, entry higher, entry lower, in turn
                    a, c = emap[k]
                    tombs.append((k,) + (((a + 1) % R, c), (a, c), (a, c - 1), (a, c + 1))[(j // 2) % 4])
                else:
                    tombs.append((k, j % R, 1 + j % 5))
            out.append(Case("readd_%d_tombs_%d_entries" % (nt, ne), R,
                            [[small_src(P[0], 0, 0)], [(0, [1, 2, 3], ents, tombs)], [small_src(P[2], 2, 0)]], P))
    return out


# ------------------------------------------------------------------ 6. kinds and coverage

def kind_cases():
    R = 4
    Pa = [5, 0, 7, TOP]
    docs = [
        ("full_empty_state", Pa, [(1, [1] * R, [], [])]),
        ("full_actor_above_R", [5, 6, 7, 8], [(R + 1, [1] * R, [(3, 0, 5), (9, 1, 1)], []),
                                              (BIG_ACTOR, [2] * R, [(4, 0, 5)], [(8, 0, 1)])]),
        ("full_entries_at_actor_R", Pa, [(1, [1] * R, [(3, R, 1), (6, 0, 5), (9, R, 9)], [])]),
        ("delta_equal_below_top", [5, 0, TOP - 1, TOP],
         [(0, [1] * R, [(1, 0, 5), (2, 0, 6), (3, 3, TOP), (4, 3, TOP - 1), (5, 2, TOP), (6, 2, TOP - 1), (7, 0, 4)], [])]),
        ("delta_entry_above_R", [5, 6, 7, 8], [(2, [1] * R, [(1, R + 1, 1), (2, 0, 5), (3, BIG_ACTOR, 1), (4, 3, 8)], [])]),
        ("delta_one_tombstone_no_entry", [5, 6, 7, 8], [(0, [1] * R, [(1, 0, 5), (2, 1, 6)], [(1, 0, 5)]),
                                                         (3, [1] * R, [], [(9, 2, 1)])]),
        ("none", [5, 6, 7, 8], [(0, [1] * R, [(1, 0, 5), (2, 1, 6)], []), (1, [1] * R, [], []),
                                (2, [1] * R, [(4, 2, 7)], [(4, 3, 1)])]),  # its one tombstone is on a key added again
        ("full_and_delta_side_by_side", Pa,
         [(0, [1] * R, [(1, 0, 5), (2, 1, 1), (3, 2, 8)], [(5, 1, 1)]),       # DELTA: P[0] = 5
          (1, [2] * R, [(1, 0, 5), (2, 1, 1), (3, 2, 7)], [(5, 1, 1)]),       # FULL: P[1] = 0, the same dots all shipped
          (2, [3] * R, [(1, 0, 6), (2, 1, 1), (3, 2, 7)], None),              # DELTA: P[2] = 7
          (3, [4] * R, [(1, 3, TOP), (2, 1, 1)], [])]),                      # DELTA: P[3] = 2^64 - 1
    ]
    names = [n for n, _, _ in docs]
    case = Case("kinds", R, [s for _, _, s in docs], [P for _, P, _ in docs])
    return [case], names


KIND_CASES, KIND_DOCS = kind_cases()


# ------------------------------------------------------------------ 7. optional arrays

def without_tombs(case, name, **kw):
    per_doc = [[(a, vv, e, None) for a, vv, e, _ in doc] for doc in case.per_doc]
    return Case(name, case.R, per_doc, case.peers, **kw)


def optional_cases():
    base = Case("", 5, [geo_doc(5, d) for d in range(14)], [clock(5, d) for d in range(14)])
    return [
        base._replace(name="kind_null", kind_null=True),
        without_tombs(base, "no_tombs_out_arrays_null", tombs="out_null"),
        without_tombs(base, "no_tombs_out_tomb_off_given", tombs="out_given"),
    ]


def all_cases() -> List[Case]:
    cases = (geometry_cases() + staging_cases() + empties_cases() + chunk_cases() + readd_cases() + KIND_CASES +
             optional_cases())
    assert len({c.name for c in cases}) == len(cases)
    return cases


CASES = all_cases()
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------ census

def masks_of(flags):
    """Per 64-position chunk (mask, valid): bit l of mask is set where position 64 * chunk + l is kept."""
    out = []
    for c0 in range(0, len(flags), CHUNK):
        part = flags[c0:c0 + CHUNK]
        out.append((sum(1 << l for l, f in enumerate(part) if f), len(part)))
    return out


def census(case: Case):
    """What the layout of a case makes the kernel walk through: per group its documents,
    sources and staged runs; per run the source starts relative to the run's first entry and
    first tombstone, the empty sources, the kinds, and per 64-position chunk the kept lanes
    as the restatement (extract_ref) gives them."""
    G = group_size(case.R)
    n_docs = len(case.per_doc)
    groups = []
    for d0 in range(0, n_docs, G):
        docs = range(d0, min(d0 + G, n_docs))
        srcs = [(d, s) for d in docs for s in case.per_doc[d]]
        runs = []
        for r0 in range(0, len(srcs), RUN):
            run = srcs[r0:r0 + RUN]
            e_starts, t_starts, e_keep, t_keep, kinds = [], [], [], [], []
            for d, s in run:
                kind, eout, tout = model.extract_ref(s, case.peers[d])
                kinds.append(kind)
                e_starts.append(len(e_keep))
                t_starts.append(len(t_keep))
                ekeys, tkeys = {e[0] for e in eout}, {t[0] for t in tout}
                e_keep += [e[0] in ekeys for e in s[2]]
                t_keep += [t[0] in tkeys for t in (s[3] or [])]
            n = len(run)
            sizes_e = [len(s[2]) for _, s in run]
            sizes_t = [len(s[3] or []) for _, s in run]
            runs.append(dict(
                n=n, kinds=kinds, e_starts=e_starts, t_starts=t_starts, e_total=len(e_keep), t_total=len(t_keep),
                e_sizes=sizes_e, t_sizes=sizes_t,
                e_empty=[i for i in range(n) if not sizes_e[i]], t_empty=[i for i in range(n) if not sizes_t[i]],
                e_kept=sum(e_keep), t_kept=sum(t_keep), e_masks=masks_of(e_keep), t_masks=masks_of(t_keep)))
        groups.append(dict(nd=len(docs), n_srcs=len(srcs), doc_srcs=[len(case.per_doc[d]) for d in docs], runs=runs))
    return dict(G=G, n_docs=n_docs, groups=groups)


def flat_peers(case: Case):
    return [x for P in case.peers for x in P]


def receiver(case: Case, d: int):
    """The receiving replica of document d, derived from the case alone: its clock is the peer
    clock, and of the keys its sources hold, in order, it has a third under the source's own
    dot, a third under another dot its clock covers, and lacks a third -- over entry and
    tombstone keys alike, so that every shipped and every withheld dot meets a present and an
    absent key.  (Actor R cannot be held: the reference panics on it.)"""
    R, P = case.R, case.peers[d]
    ents, n = {}, 0
    for _a, _vv, e, t in case.per_doc[d]:
        for k, a, c in list(e) + list(t or []):
            if k in ents:
                continue
            n += 1
            if n % 3 == 0:
                ents[k] = (a if a != R else 0, c)
            elif n % 3 == 1:
                b = n % R
                ents[k] = (b, max(P[b], 1))
    return sorted((k, a, c) for k, (a, c) in ents.items()), list(P)


def expected(case: Case):
    """(kinds over all sources, the message per document) by the restatement."""
    kinds, msgs = [], []
    for d, sources in enumerate(case.per_doc):
        k, m = model.extract_doc_ref(sources, case.peers[d])
        kinds += k
        msgs.append(m)
    return kinds, msgs
