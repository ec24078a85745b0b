"""Shared by tests/test_fold_log_model.py (CPU) and tests/test_gpu_fold_log.py:
fold_log_ref, the expectation of crdt_awset_fold_log_async (include/crdtgpu.h),
the path a document takes through csrc/fold_log.hip, and the hand-built case table.

fold_log_ref(mode, dst, srcs) is the C oracle's fold (oracle.fold) and then
diff_doc of tests/test_diff_model.py on (dst, out), document by document, laid
out as the call lays it out: document d's removed list at dst.offsets[d], its
upserted list at entry_off[doc_srcs[d]], the merged state at the sum of the two.
Nothing in it comes from the code under test.

A document is (dst entries [(key, actor, counter)], dst vv, chain) with chain =
[(actor, vv, entries, tombstones)], as in tests/fold_edge_cases.py; counters and
clock values stay within 0..MAX_C so that tests/counter_maps.py can push the
same cases up to the 64-bit edges.
"""

from typing import Dict, List, NamedTuple

import numpy as np

from crdtgpu import CRDT_FOLD_AWSET, CRDT_FOLD_DELTA
from crdtgpu.batch import AWSetBatch, SrcBatch
from join_log_cases import LogRef, _slots_idx
from oracle import awset_ref as ref
from oracle import oracle
from test_diff_model import ADDED, CLOCK, REMOVED, UPDATED, diff_doc

AWSET, DELTA = CRDT_FOLD_AWSET, CRDT_FOLD_DELTA
U8, U32, U64 = np.uint8, np.uint32, np.uint64
MAX_C = 9          # counters and clock values of every case here lie in 0..MAX_C
WAVE_MAX = 64      # kFoldLogWaveMax: entries of any list, and of the running state, on the wave path
LOG_WAVES = 4      # kFoldLogWaves: wavefronts per workgroup of the wave path
LOG_DOCS = 4       # kFoldLogDocs: consecutive documents one wavefront takes in turn
WINDOW = 1024      # kFoldLogBlockNT * kFoldLogBlockIPT: merged positions per step of the block path
TOP = 2 ** 64 - 1


# ------------------------------------------------------------------ reference

def ups_offsets_of(srcs):
    return np.asarray(srcs.entry_off, U32)[np.asarray(srcs.doc_srcs).astype(np.int64)]


def fold_log_of(dst, srcs, after):
    """The log of the fold of srcs into dst given the folded batch `after`: diff_doc per
    document, in the call's layout.  The asserts are the capacity bounds of the two lists."""
    n, R = dst.n_docs, dst.R
    ds, es = int(dst.offsets[-1]), int(np.asarray(srcs.entry_off)[-1])
    uo = ups_offsets_of(srcs)
    log = {"flags": np.zeros(n, U8), "summary": np.zeros(5, U32),
           "rem_offsets": np.asarray(dst.offsets, U32).copy(), "rem_counts": np.zeros(n, U32),
           "rem_keys": np.zeros(ds, U64), "rem_actors": np.zeros(ds, U32), "rem_counters": np.zeros(ds, U64),
           "ups_offsets": uo.copy(), "ups_counts": np.zeros(n, U32),
           "ups_keys": np.zeros(es, U64), "ups_actors": np.zeros(es, U32), "ups_counters": np.zeros(es, U64),
           "ups_kind": np.zeros(es, U8)}
    n_upd = 0
    for d in range(n):
        r, u, k = diff_doc(dst, after, d)
        f = (REMOVED if len(r[0]) else 0) | (ADDED if (k == ADDED).any() else 0) | (UPDATED if (k == UPDATED).any() else 0)
        if (np.asarray(dst.vv[d * R:(d + 1) * R]) != np.asarray(after.vv[d * R:(d + 1) * R])).any():
            f |= CLOCK
        log["flags"][d] = f
        o, m = int(dst.offsets[d]), len(r[0])
        assert o + m <= int(dst.offsets[d + 1])  # a removed entry was a dst entry
        log["rem_counts"][d] = m
        for col, v in zip(("rem_keys", "rem_actors", "rem_counters"), r):
            log[col][o:o + m] = v
        o, m = int(uo[d]), len(u[0])
        assert o + m <= int(uo[d + 1]), "document %d: %d upserts, %d source entry slots" % (d, m, int(uo[d + 1]) - o)
        log["ups_counts"][d] = m
        for col, v in zip(("ups_keys", "ups_actors", "ups_counters", "ups_kind"), u + (k,)):
            log[col][o:o + m] = v
        n_upd += int((k == UPDATED).sum())
    fl = log["flags"]
    log["summary"][:] = [int(log["rem_counts"].sum()), int(log["ups_counts"].sum()), n_upd,
                         int(((fl & 7) != 0).sum()), int((fl != 0).sum())]
    return log


def fold_log_ref(mode, dst, srcs):
    dst, srcs = dst.numpy(), srcs.numpy()
    rc, out = oracle.fold(mode, dst, srcs)
    log = fold_log_of(dst, srcs, out.as_batch())
    return LogRef(rc, out, log, _slots_idx(log["rem_offsets"], log["rem_counts"]),
                  _slots_idx(log["ups_offsets"], log["ups_counts"]))


# ----------------------------------------------------- the steps, one at a time, on maps

def doc_of(dst, srcs, d):
    """Document d of a batch pair as (entries, vv, chain), live prefixes only."""
    dst, srcs = dst.numpy(), srcs.numpy()
    R = dst.R
    e, vv = dst.doc(d)
    chain = []
    for s in range(int(srcs.doc_srcs[d]), int(srcs.doc_srcs[d + 1])):
        a, b = int(srcs.entry_off[s]), int(srcs.entry_off[s + 1])
        ents = list(zip(srcs.keys[a:b].tolist(), srcs.actors[a:b].tolist(), srcs.counters[a:b].tolist()))
        tombs = []
        if srcs.tomb_off is not None:
            a, b = int(srcs.tomb_off[s]), int(srcs.tomb_off[s + 1])
            tombs = list(zip(srcs.tkeys[a:b].tolist(), srcs.tactors[a:b].tolist(), srcs.tcounters[a:b].tolist()))
        chain.append((int(srcs.src_actor[s]), [int(x) for x in srcs.vv[s * R:(s + 1) * R]], ents, tombs))
    return [tuple(int(x) for x in t) for t in e], [int(x) for x in vv], chain


def replay(mode, entries, vv, chain):
    """(entries after, vv after, live entries after every step): the reference's own
    (*AWSet).Merge / (*AWSetDelta).Merge, step by step, on maps (oracle/awset_ref.py)."""
    dots = lambda es: {k: ref.Dot(a, c) for k, a, c in es}  # noqa: E731
    cur = (ref.AWSetDelta if mode == DELTA else ref.AWSet)(0, list(vv), dots(entries))
    sizes = []
    for actor, svv, ents, tombs in chain:
        if mode == DELTA:
            cur.Merge(ref.AWSetDelta(actor, list(svv), dots(ents), dots(tombs) or None))
        else:
            cur.Merge(ref.AWSet(actor, list(svv), dots(ents)))
        sizes.append(len(cur.Entries))
    after = sorted((k, d.actor, d.counter) for k, d in cur.Entries.items())
    return after, list(cur.VersionVector), sizes


def path_of(mode, entries, vv, chain, tombs_given=True):
    """"wave", "block" (dst alone is too large) or ("bail", k): the wave path gives the
    document up at step k, where a source's entries or tombstones, or the state after
    the step, pass WAVE_MAX."""
    if len(entries) > WAVE_MAX:
        return "block"
    sizes = replay(mode, entries, vv, chain)[2]
    for k, (_, _, ents, tombs) in enumerate(chain):
        nt = len(tombs) if (mode == DELTA and tombs_given) else 0
        if len(ents) > WAVE_MAX or nt > WAVE_MAX or sizes[k] > WAVE_MAX:
            return ("bail", k)
    return "wave"


# ------------------------------------------------------------------- the cases

class Case(NamedTuple):
    name: str
    mode: int
    R: int
    docs: List[tuple]          # (entries, vv, chain)
    paths: Dict[int, object]   # document -> the path it is built for
    edges: tuple               # the named edges of the issue the case reaches


def batches(case, slack=0):
    dst = AWSetBatch.from_docs(case.R, [(e, vv) for e, vv, _ in case.docs], slack=slack)
    return dst, SrcBatch.from_lists(case.R, [c for _, _, c in case.docs])


def seq(n, start=1, step=3, actor=0, c=1):
    return [(start + step * i, actor, c) for i in range(n)]


V = [5, 5]           # dst's clock in the R = 2 cases: counters up to 5 are seen, above are new
A0 = (10, 0, 3)      # a dst entry under a dot of actor 0 that clocks [4, .] and above cover
PADS = seq(3, 100)   # bystanders under a seen dot: common keys that stay as they are


def net_effect_cases():
    cs = []
    base = [A0] + PADS

    def S(actor, vv, ents, tombs=()):
        return (actor, list(vv), sorted(list(ents) + PADS), sorted(tombs))

    def add(name, mode, dst, vv, chain, edge):
        cs.append(Case(name, mode, 2, [(sorted(dst), list(vv), chain)], {0: "wave"}, (edge,)))

    for mode in (AWSET, DELTA):
        m = "awset" if mode == AWSET else "delta"
        # removed at step 0 (AWSet: the source's clock covers the dot; delta: a tombstone dst has not
        # seen), back at step 1 under another dot
        gone = S(1, [4, 0], []) if mode == AWSET else S(1, [5, 6], [], [(10, 1, 6)])
        add("readd_other_dot_" + m, mode, base, V, [gone, S(1, [0, 9], [(10, 1, 9)])], "removed then re-added, another dot")
        # added at step 0, gone at step 1
        drop = S(0, [0, 8], []) if mode == AWSET else S(0, [6, 8], [], [(20, 0, 6)])
        add("add_then_remove_" + m, mode, base, V, [S(1, [0, 7], [(20, 1, 7)]), drop], "added then removed")
        # moved to another dot at step 0, gone at step 1: one removed record, with dst's dot
        drop = S(0, [0, 8], []) if mode == AWSET else S(0, [6, 8], [], [(10, 0, 6)])
        add("update_then_remove_" + m, mode, base, V, [S(1, [0, 7], [(10, 1, 7)]), drop], "updated then removed")
        # two updates: one UPDATED, the last dot
        add("two_updates_" + m, mode, base, V, [S(1, [0, 7], [(10, 1, 7)]), S(1, [0, 8], [(10, 1, 8)])], "two updates")
    # removed at step 0, back under the same dot: only a tombstone can remove an entry whose dot the
    # running clock still lacks afterwards, so dst holds 10 under (1, 7), which its own clock has not seen
    add("readd_same_dot_delta", DELTA, [(10, 1, 7)] + PADS, V,
        [S(0, [6, 5], [], [(10, 0, 6)]), S(0, [6, 5], [(10, 1, 7)])], "removed then re-added, same dot")
    # an AWSet step always takes the source's dot of a common key, so an update can come back to dst's own
    add("update_returns_awset", AWSET, base, V, [S(1, [0, 7], [(10, 1, 7)]), S(0, [0, 0], [A0])], "update returns to dst's dot")
    add("tomb_removes_added_delta", DELTA, base, V, [S(1, [5, 7], [(20, 1, 7)]), S(1, [5, 8], [], [(20, 1, 8)])],
        "a tombstone of step j' removes a key step j added")
    # nothing of the source is new to dst, its clock is ahead: NONE, not even the clock moves
    add("none_step_delta", DELTA, base, V, [(1, [9, 9], sorted(base), [])], "a NONE step leaves the clock alone")
    # first contact: dst's clock holds 0 for the source's actor
    add("first_contact_clock_only_delta", DELTA, base, [5, 0], [(1, [7, 0], sorted(base), [])], "FULL, CLOCK only")
    add("first_contact_clock_clear_delta", DELTA, base, [5, 0], [(1, [3, 0], sorted(base), [])], "FULL, CLOCK clear")
    return cs


def grow_doc(n0, adds, mode=AWSET, key0=1):
    """dst holds n0 keys; step k brings adds[k] fresh keys under dots nobody has seen (the
    sources' clocks cover nothing of dst: an AWSet step removes none of its keys)."""
    dst = seq(n0, key0)
    chain, nxt = [], key0 + 3 * n0
    for k, a in enumerate(adds):
        chain.append((1, [0, 6], [(nxt + 3 * i, 1, 7 + (k % 3)) for i in range(a)], []))
        nxt += 3 * a
    return dst, list(V), chain


def threshold_cases():
    cs = []
    for mode in (AWSET, DELTA):
        m = "awset" if mode == AWSET else "delta"
        # dst live 63 / 64 / 65, one small source
        docs = [(seq(n), list(V), [(1, [0, 6], [(2, 1, 6)], [])]) for n in (63, 64, 65)]
        # (63 + 1 = 64 stays; 64 + 1 = 65 is given up at step 0)
        cs.append(Case("dst_live_" + m, mode, 2, docs, {0: "wave", 1: ("bail", 0), 2: "block"}, ("dst live 63/64/65",)))
        # one source's entries 63 / 64 / 65, all common with dst or seen: the state stays small
        docs = []
        for n in (63, 64, 65):
            docs.append(([(1, 0, 1)], list(V), [(1, [0, 5], [(4, 1, 6)], []), (1, [0, 6], seq(n, 1, 3, 1, 2), [])]))
        cs.append(Case("src_entries_" + m, mode, 2, docs, {0: "wave", 1: "wave", 2: ("bail", 1)},
                       ("source entries 63/64/65",)))
        # the running state 64 -> 65 at the first, a middle and the last step, and staying at 64
        docs = [grow_doc(64, [1, 1, 1], mode), grow_doc(62, [2, 1, 1], mode), grow_doc(61, [1, 2, 1], mode),
                grow_doc(61, [1, 1, 1], mode)]
        cs.append(Case("state_grows_" + m, mode, 2, docs, {0: ("bail", 0), 1: ("bail", 1), 2: ("bail", 2), 3: "wave"},
                       ("running state 64 -> 65",)))
        # a document that is given up, and a small one after it on the same wavefront
        docs = [grow_doc(62, [2, 1], mode), ([(5, 0, 1)], list(V), [(1, [5, 7], [(8, 1, 7)], [])]),
                grow_doc(65, [1], mode), ([], list(V), [(1, [5, 7], [(8, 1, 7)], [])])]
        cs.append(Case("stale_lds_" + m, mode, 2, docs, {0: ("bail", 1), 1: "wave", 2: "block", 3: "wave"},
                       ("a small document after one that bails",)))
    # one source's tombstones 63 / 64 / 65 (of keys dst holds, under dots it has not seen: removed)
    docs = []
    for n in (63, 64, 65):
        docs.append((seq(40), list(V), [(1, [5, 6], [(500, 1, 6)], seq(n, 1, 3, 1, 6))]))
    cs.append(Case("src_tombs_delta", DELTA, 2, docs, {0: "wave", 1: "wave", 2: ("bail", 0)}, ("source tombstones 63/64/65",)))
    # the same tombstones under CRDT_FOLD_AWSET: not read, not counted
    cs.append(Case("src_tombs_awset", AWSET, 2, docs, {0: "wave", 1: "wave", 2: "wave"}, ("tombstones in AWSET mode",)))
    return cs


def big_doc(mode, nd=1500, ns=1300, salt=0):
    """A block-path document of two windows and a half: removes, adds, updates over three steps."""
    dst = [(3 * i + 1, i % 2, 1 + (i % 5)) for i in range(nd)]
    s0 = [(3 * i + 1 + (i % 2), 1, 6 + (i % 3)) for i in range(0, ns)]            # half common (moved), half new
    s1 = [(3 * i + 1, 0, 7) for i in range(0, nd, 7)]                            # common: moved again
    t1 = [(3 * i + 1, 1, 9) for i in range(3, nd, 11)] if mode == DELTA else []  # removed by tombstones
    return dst, [5, 5], [(1, [5 + salt, 8], s0, []), (0, [8, 8], s1, t1), (1, [9, 9], [], [])]


def shape_cases():
    cs = []
    small = (1, [5, 7], [(8, 1, 7)], [])
    empty = (1, [5, 6], [], [])
    for mode in (AWSET, DELTA):
        m = "awset" if mode == AWSET else "delta"
        docs = [(seq(4), list(V), []),                                   # no sources: out = dst, empty lists, flags 0
                ([], list(V), [small]),                                  # empty dst
                ([], list(V), []),                                       # nothing at all
                (seq(4), list(V), [empty, small, (1, [5, 8], [(11, 1, 8)], [])]),   # an empty source first
                (seq(4), list(V), [small, empty, (1, [5, 8], [(11, 1, 8)], [])]),   # in the middle
                (seq(4), list(V), [small, (1, [5, 8], [(11, 1, 8)], []), empty]),   # last
                ([(0, 0, 1), (2 ** 63, 0, 2), (TOP, 0, 9)], list(V),
                 [(1, [5, 7], [(0, 1, 7), (2 ** 63 - 1, 1, 6), (TOP, 1, 7)], [])])]  # keys 0, 2^63, 2^64 - 1
        cs.append(Case("shapes_" + m, mode, 2, docs, {i: "wave" for i in range(len(docs))},
                       ("no sources", "empty dst", "empty sources first / middle / last", "keys 0, 2^63, 2^64 - 1")))
        cs.append(Case("one_document_" + m, mode, 2, [(seq(4), list(V), [small])], {0: "wave"}, ("one document",)))
        cs.append(Case("block_" + m, mode, 2, [big_doc(mode), (seq(3), list(V), [small]), big_doc(mode, 700, 90, 1)],
                       {0: "block", 1: "wave", 2: "block"}, ("block path, several windows",)))
    return cs


def width_cases():
    """R = 1, 2, 3 and 64: seeded documents of tests/fold_edge_cases.py's builder (a handful of
    sources, adds, skips, moved dots, removals, and for delta folds first contacts and no-ops)."""
    import random

    import fold_edge_cases as fe

    cs = []
    for mode in (AWSET, DELTA):
        for R in (1, 2, 3, 64):
            rng = random.Random(4100 + 10 * R + mode)
            docs = []
            for d in range(40):
                feature = (None, "first", "noop")[d % 3] if mode == DELTA else None
                nd = 70 if d % 13 == 5 else rng.randint(0, 20)
                docs.append(fe.make_doc(rng, R, mode == DELTA, rng.randint(0, 6), nd, list(range(100 * d, 100 * d + 90)),
                                        ents=(0, 6), tombs=(0, 3), feature=feature))
            cs.append(Case("width_R%d_%s" % (R, "awset" if mode == AWSET else "delta"), mode, R, docs, {}, ("R = %d" % R,)))
    return cs


def many_docs_case(mode, n=LOG_WAVES * LOG_DOCS * 40 + 3):
    """More documents than one workgroup's sixteen, no multiple of them; every 50th is a block-path one."""
    docs = []
    for d in range(n):
        k = 8 * d
        if d % 50 == 17:
            docs.append((seq(70, k * 100 + 1), list(V), [(1, [5, 7], [(k * 100 + 2, 1, 7)], [])]))
        else:
            docs.append(([(k, d % 2, 1 + d % 5), (k + 1, 0, 3)], list(V),
                         [(1, [4 + d % 3, 6], [(k, 1, 6), (k + 2, 1, 6 + d % 2)], [(k + 1, 1, 7)] if d % 3 == 0 else [])]))
    return Case("many_docs_" + ("awset" if mode == AWSET else "delta"), mode, 2, docs, {0: "wave", 17: "block"},
                ("more documents than a workgroup has wavefronts",))


_cases = None


def all_cases():
    """name -> Case, built once (never modified by a test).  fold_edge_cases.all_cases() is
    run beside these by the GPU test, in its own batches."""
    global _cases
    if _cases is None:
        cs = net_effect_cases() + threshold_cases() + shape_cases() + width_cases()
        cs += [many_docs_case(AWSET), many_docs_case(DELTA)]
        _cases = {c.name: c for c in cs}
        assert len(_cases) == len(cs)
    return _cases


NAMED_EDGES = ("removed then re-added, same dot", "removed then re-added, another dot", "added then removed",
               "updated then removed", "update returns to dst's dot", "two updates",
               "a tombstone of step j' removes a key step j added", "a NONE step leaves the clock alone",
               "FULL, CLOCK only", "FULL, CLOCK clear", "dst live 63/64/65", "source entries 63/64/65",
               "source tombstones 63/64/65", "tombstones in AWSET mode", "running state 64 -> 65",
               "a small document after one that bails", "no sources", "empty dst", "empty sources first / middle / last",
               "keys 0, 2^63, 2^64 - 1", "one document", "block path, several windows", "R = 1", "R = 2", "R = 3", "R = 64",
               "more documents than a workgroup has wavefronts")
