"""A census of the paths a fold batch takes through csrc/fold.hip, on the CPU.

fold.hip's dispatch -- which pass folds a document (the lean slot walk, the
general kernel directly or from the deferred list, the block kernel), why a
document left the pass before, how its tombstones' re-add check runs, whether
the clock schedule is replayed, which sort tier its kept tuples take -- is
decided by a handful of thresholds.  They are restated here in one table, each
with the fold.hip line it comes from, and classify() applies them to a batch the
way the kernels do.

This is a restatement, not a measurement: it does not ask the kernel which way
it went.  Its use is to make the deterministic cases of tests/fold_edge_cases.py
land on every edge on purpose, and to make tests/test_fold_paths_model.py fail
when a case stops doing so.  A change of a threshold in fold.hip updates the
table below.

The general delta kernel's dense_delta_walk looks at the key span of the *kept*
tuples only.  The census takes the kept set from its own replay of the schedule;
the case builders do not lean on that: a "dense" case keeps every tuple of a
document within the limit, a "wide" case puts the span into the document's own
entries, which are always kept.  (dense_sort's span test, inside the sort path,
is not told apart here: `resolve` is slot-walk or sort.)
"""

from __future__ import annotations

from collections import Counter

import numpy as np

from crdtgpu import CRDT_FOLD_AWSET, CRDT_FOLD_DELTA

AWSET, DELTA = CRDT_FOLD_AWSET, CRDT_FOLD_DELTA

# ---------------------------------------------------------------- thresholds
# name: (value, "fold.hip line(s)", what it bounds)
THRESHOLDS = {
    "NCAP_AWSET": (128, "100, 979, 1053", "tuples n + E + X of a document on the pipe kernels, AWSet folds (64 * NCH, NCH 2)"),
    "NCAP_DELTA": (256, "100, 979, 1053", "the same for delta folds (NCH 4)"),
    "MCAP": (64, "112, 1054", "sources of a document on the general pipe kernel"),
    "LEAN_MS": (15, "377, 499, 666, 1054", "sources of a document in a lean pass and in the slot walks"),
    "VCAP_AWSET_LEAN": (64, "105, 1054", "clock words sources x R, lean AWSet pass"),
    "VCAP_AWSET": (128, "105, 1054", "clock words, general AWSet kernel"),
    "VCAP_DELTA_LEAN": (192, "105, 1054", "clock words, lean delta pass"),
    "VCAP_DELTA": (256, "105, 1054", "clock words, general delta kernel (3 waves per SIMD)"),
    "SPAN_AWSET": (64, "392", "dense_awset_walk: key span of all tuples must be below it"),
    "SPAN_DELTA": (256, "253, 526, 694", "dense_delta_walk, fused_delta_walk, dense_sort: key span below it"),
    "STEP_TABLE_MS": (32, "246, 1388", "sources up to which the re-add step table (and dense_sort) is used"),
    "KC_TIER_1": (64, "1537, 1541", "kept tuples sorted one per lane"),
    "KC_TIER_2": (128, "1538", "kept tuples sorted two per lane (delta folds: four beyond)"),
    "PACK_32": (1 << 15, "wave_sort.hpp:175", "key range for the 32-bit (key, tag) packing of the in-register sort"),
    "PACK_64": (1 << 47, "wave_sort.hpp:176", "key range for its 64-bit packing (80-bit comparison beyond)"),
    "K_AWSET": (32, "942, 958", "consecutive documents per wavefront, AWSet folds"),
    "K_DELTA": (8, "945, 959", "consecutive documents per wavefront, delta folds"),
    "WAVES_AWSET": (2, "939, 952", "wavefronts per workgroup, AWSet folds"),
    "WAVES_DELTA": (1, "948, 953", "wavefronts per workgroup, delta folds"),
    "XCDS": (8, "1016", "the lean AWSet pass renumbers its workgroups over this many XCDs"),
}


def T(name):
    return THRESHOLDS[name][0]


PASSES = ("lean", "general-direct", "general-deferred", "block")
MS_BANDS = ("0", "1..15", "16..32", "33..63", "64", ">64")
WHYS = ("tuples", "sources>15", "sources>64", "clocks", "span", "full-step", "noop-step", "actor==R", "empty")
KC_TIERS = ("<=64", "<=128", ">128")


def ncap(mode):
    return T("NCAP_DELTA") if mode == DELTA else T("NCAP_AWSET")


def vcap(mode, lean):
    return T(("VCAP_DELTA" if mode == DELTA else "VCAP_AWSET") + ("_LEAN" if lean else ""))


def docs_per_workgroup(mode):
    return (T("K_DELTA") * T("WAVES_DELTA")) if mode == DELTA else (T("K_AWSET") * T("WAVES_AWSET"))


def ms_band(ms):
    if ms == 0:
        return "0"
    if ms <= 15:
        return "1..15"
    if ms <= 32:
        return "16..32"
    if ms <= 63:
        return "33..63"
    return "64" if ms == 64 else ">64"


def kc_tier(mode, kc):
    if kc <= T("KC_TIER_1"):
        return "<=64"
    if mode == AWSET or kc <= T("KC_TIER_2"):
        return "<=128"
    return ">128"


def span_of(keys):
    """max - min of a key list in plain integers (no wrap), -1 when empty."""
    return max(keys) - min(keys) if keys else -1


def big_why(mode, lean, N, ms, R):
    """fold.hip:1053-1054, the hand-off test of a pipe kernel (None: the document stays)."""
    if N > ncap(mode):
        return "tuples"
    if ms > (T("LEAN_MS") if lean else T("MCAP")):
        return "sources>15" if lean else "sources>64"
    if ms * R > vcap(mode, lean):
        return "clocks"
    return None


def doc_lists(dst, srcs, d, tombs=True):
    """(entries, vv, chain) of document d of host batches; chain[j] = (actor, vv, entries,
    tombstones).  A live count above the slots is clamped to them, as the kernels do."""
    R = dst.R
    o, slots = int(dst.offsets[d]), int(dst.offsets[d + 1]) - int(dst.offsets[d])
    n = slots if dst.counts is None else min(int(dst.counts[d]), slots)
    ents = list(zip(dst.keys[o:o + n].tolist(), dst.actors[o:o + n].tolist(), dst.counters[o:o + n].tolist()))
    chain = []
    for k in range(int(srcs.doc_srcs[d]), int(srcs.doc_srcs[d + 1])):
        e0, e1 = int(srcs.entry_off[k]), int(srcs.entry_off[k + 1])
        e = list(zip(srcs.keys[e0:e1].tolist(), srcs.actors[e0:e1].tolist(), srcs.counters[e0:e1].tolist()))
        t = []
        if tombs and srcs.tomb_off is not None:
            t0, t1 = int(srcs.tomb_off[k]), int(srcs.tomb_off[k + 1])
            t = list(zip(srcs.tkeys[t0:t1].tolist(), srcs.tactors[t0:t1].tolist(), srcs.tcounters[t0:t1].tolist()))
        chain.append((int(srcs.src_actor[k]), srcs.vv[k * R:(k + 1) * R].tolist(), e, t))
    return ents, dst.vv[d * R:(d + 1) * R].tolist(), chain


def has_dot(vv, a, c):
    return a < len(vv) and vv[a] >= c


def schedule(mode, vv0, chain):
    """The clock schedule as the kernels run it (fold.hip:1280-1310, 1441-1495).

    First under the prefix-max clocks U_j (no step assumed a no-op): full_j, the
    changed entries, the effective tombstones, hence the no-op steps.  If there is
    one, the general kernel replays the steps one at a time with the exact clocks.
    Returns a dict: full_u / noop_u (lists under U), replay (bool), full / noop /
    changed (exact: after the replay when there was one), eff[(j, x)], and
    readd[(j, x)] for the tombstones whose key has an entry in their own source
    (True: re-added, the tombstone is dropped -- the two verdicts of :1433)."""
    R = len(vv0)
    delta = mode == DELTA
    eff, readd = {}, {}
    for j, (_, _, e, t) in enumerate(chain):
        emap = {k: (a, c) for k, a, c in e}
        for x, (k, a, c) in enumerate(t):
            s = emap.get(k)
            if s is not None:
                readd[(j, x)] = s[0] != a or s[1] > c
            eff[(j, x)] = not (s is not None and (s[0] != a or s[1] > c))

    def run(exact):
        V = list(vv0)
        full, noop, chg = [], [], {}
        for j, (aj, svv, e, t) in enumerate(chain):
            f = (not delta) or (V[aj] if aj < R else 0) == 0
            nop = False
            if not f:
                anyc = False
                for i, (k, a, c) in enumerate(e):
                    chg[(j, i)] = not has_dot(V, a, c)
                    anyc |= chg[(j, i)]
                nop = not anyc and not any(eff[(j, x)] for x in range(len(t)))
            full.append(f)
            noop.append(nop)
            if not (exact and nop):
                V = [max(x, y) for x, y in zip(V, svv)]
        return full, noop, chg

    full_u, noop_u, chg_u = run(False)
    replay = delta and any(noop_u)
    full, noop, chg = run(True) if replay else (full_u, noop_u, chg_u)
    return dict(full_u=full_u, noop_u=noop_u, replay=replay, full=full, noop=noop, changed=chg, eff=eff, readd=readd)


def classify_doc(mode, lean_first, ents, vv0, chain):
    """The path record of one document (see classify)."""
    delta = mode == DELTA
    R = len(vv0)
    n, ms = len(ents), len(chain)
    E = sum(len(s[2]) for s in chain)
    X = sum(len(s[3]) for s in chain) if delta else 0
    N = n + E + X
    keys_all = [k for k, _, _ in ents] + [k for s in chain for k, _, _ in s[2]] + \
        ([k for s in chain for k, _, _ in s[3]] if delta else [])
    actors_all = [a for _, a, _ in ents] + [a for s in chain for _, a, _ in s[2]] + \
        ([a for s in chain for _, a, _ in s[3]] if delta else [])
    sch = schedule(mode, vv0, chain)
    rec = dict(n=n, ms=ms, E=E, X=X, N=N, R=R, ms_band=ms_band(ms), why=None, lean_why=None, tomb_search=None,
               noop_replay=False, kc_tier=None, kc=None, resolve=None, readd=(), seq_walk=False)

    # ---- the lean pass (fold.hip:1369-1379 delta, 1499-1510 AWSet)
    if lean_first:
        why = big_why(mode, True, N, ms, R)
        if why is None and delta:
            if any(sch["full_u"]):
                why = "full-step"
            elif N == 0:
                why = "empty"
            elif R in actors_all:
                why = "actor==R"
            elif span_of(keys_all) >= T("SPAN_DELTA"):
                why = "span"
            elif any(sch["noop_u"]):
                why = "noop-step"
        elif why is None:
            if N == 0:
                why = "empty"
            elif span_of(keys_all) >= T("SPAN_AWSET"):
                why = "span"
        if why is None:
            rec.update({"pass": "lean", "resolve": "slot-walk", "tomb_search": "table" if X else None,
                        "seq_walk": (not delta) and R in actors_all})
            if delta:
                rec["readd"] = tuple(sorted(set(sch["readd"].values())))
            return rec
        rec["lean_why"] = why

    # ---- the general kernel (every document, or the deferred list) and the block kernel behind it
    why = big_why(mode, False, N, ms, R)
    if why is not None:
        rec.update({"pass": "block", "why": why})
        return rec
    rec["pass"] = "general-deferred" if lean_first else "general-direct"
    rec["why"] = rec["lean_why"]
    if delta and X:
        rec["tomb_search"] = "table" if ms <= T("STEP_TABLE_MS") else "binary"
        rec["readd"] = tuple(sorted(set(sch["readd"].values())))
    rec["noop_replay"] = sch["replay"]
    kept_keys = [k for k, _, _ in ents]
    kept_actors = [a for _, a, _ in ents]
    for j, (_, _, e, t) in enumerate(chain):
        if sch["noop"][j]:
            continue
        for i, (k, a, c) in enumerate(e):
            if sch["full"][j] or sch["changed"].get((j, i), False):
                kept_keys.append(k)
                kept_actors.append(a)
        if delta and not sch["full"][j]:
            for x, (k, a, c) in enumerate(t):
                if sch["eff"][(j, x)]:
                    kept_keys.append(k)
                    kept_actors.append(a)
    rec["kc"] = len(kept_keys)
    rec["kc_tier"] = kc_tier(mode, rec["kc"])
    if not delta:
        walk = N > 0 and ms <= T("LEAN_MS") and span_of(keys_all) < T("SPAN_AWSET")
        rec["resolve"] = "slot-walk" if walk else "sort"
        rec["seq_walk"] = walk and R in actors_all
    elif ms > T("LEAN_MS") or not kept_keys or R in kept_actors:
        rec["resolve"] = "sort"
    else:
        rec["resolve"] = "slot-walk" if span_of(kept_keys) < T("SPAN_DELTA") else "sort"
    return rec


def classify(mode, lean_first, dst, srcs):
    """Per document of the batch, a dict with
      pass         lean / general-direct / general-deferred / block
      why          for the last two: what sent the document there (WHYS; `empty`: a
                   lean pass walks no document without tuples, fold.hip:377, 666)
      lean_why     why the lean pass left it (also kept when the block kernel takes it)
      ms_band      one of MS_BANDS
      tomb_search  table / binary / None (no tombstones): how the re-add check finds a
                   tombstone's source entries (fold.hip:1388, 1419-1435)
      readd        the verdicts of the re-add comparison (:1433) met in the document
      noop_replay  the general kernel replays the schedule step by step (:1449)
      kc, kc_tier  kept tuples and their sort tier (general kernel)
      resolve      slot-walk / sort (general kernel; the lean passes only walk)
      seq_walk     the AWSet slot walk takes its step-by-step form (an actor == R)
    and the sizes n, ms, E, X, N, R."""
    dst, srcs = dst.numpy(), srcs.numpy()
    out = []
    for d in range(dst.n_docs):
        ents, vv0, chain = doc_lists(dst, srcs, d)
        out.append(classify_doc(mode, bool(lean_first), ents, vv0, chain))
    return out


def census(records):
    """Counter over the class names a record belongs to (the census table's lines)."""
    c = Counter()
    for r in records:
        c["pass=%s" % r["pass"]] += 1
        c["pass=%s ms=%s" % (r["pass"], r["ms_band"])] += 1
        if r["why"]:
            c["why=%s" % r["why"]] += 1
        if r["pass"] == "block" and r["lean_why"]:
            c["lean_why=%s then block" % r["lean_why"]] += 1
        if r["tomb_search"]:
            c["tomb_search=%s" % r["tomb_search"]] += 1
            for v in r["readd"]:
                c["tomb_search=%s readd=%s" % (r["tomb_search"], v)] += 1
        if r["noop_replay"]:
            c["noop_replay"] += 1
            if r["ms"] > T("LEAN_MS"):
                c["noop_replay ms>15"] += 1
        if r["resolve"]:
            c["resolve=%s" % r["resolve"]] += 1
        if r["resolve"] == "sort":
            c["sort kc_tier=%s" % r["kc_tier"]] += 1
        if r["seq_walk"]:
            c["seq_walk"] += 1
    return c


def run_edges(mode, lean_first, n_docs):
    """The run and grid geometry of the first pass over n_docs documents: (workgroups,
    documents of the last run, whether the lean AWSet pass renumbers unevenly).
    fold.hip:1015-1021, 1677-1678."""
    k = T("K_DELTA") if mode == DELTA else T("K_AWSET")
    grid = -(-n_docs // docs_per_workgroup(mode))
    last = n_docs % k or k
    return grid, last, bool(lean_first) and mode == AWSET and grid % T("XCDS") != 0


def arrays_equal_live(a, b, n_docs, R):
    """None, or the first document whose live output differs between two outputs."""
    for d in range(n_docs):
        oa, ob, ca, cb = int(a.offsets[d]), int(b.offsets[d]), int(a.counts[d]), int(b.counts[d])
        if ca != cb or not (np.array_equal(a.keys[oa:oa + ca], b.keys[ob:ob + cb]) and
                            np.array_equal(a.actors[oa:oa + ca], b.actors[ob:ob + cb]) and
                            np.array_equal(a.counters[oa:oa + ca], b.counters[ob:ob + cb]) and
                            np.array_equal(a.vv[d * R:(d + 1) * R], b.vv[d * R:(d + 1) * R])):
            return d
    return None
