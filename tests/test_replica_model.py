"""CPU: replica select and scatter (crdt_replica_select_async,
crdt_replica_scatter_async) restated over the packed layout.

replica_select_ref / replica_scatter_ref are the expectation of the GPU calls
(tests/test_gpu_replica.py): vectorised numpy restatements of the contract in
include/crdtgpu.h.  They are pinned here by the calls they extend -- the state
part is select_ref (tests/test_compare_model.py) and scatter_ref
(tests/test_scatter_model.py) on every case the GPU file uses -- and by the two
rounds they close: the sparse apply (select, apply, scatter) is the apply over
the whole batch, and the sparse delta round (select both replicas, delta
exchange, scatter both) is the full delta exchange, both against the C oracle.
"""

import os
import random
import re

import numpy as np

import crdtgpu
from apply_cases import make_case
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch, OpBatch, Replica, TombBatch
from delta_pair_cases import delta_pair_ref
from helpers import PKG
from oracle import oracle
from sources_cases import make_replica, rand_docs, rand_replicas, tiny_replicas
from test_compare_model import select_ref
from test_scatter_model import same_batch, scatter_ref

U32, U64 = np.uint32, np.uint64
K_SCAN = 1024     # kRepScanChunk: output documents per workgroup of the offset scan
K_PART = 1024     # kRepPartStep: partial sums per step of the partials scan
K_GATHER = 2048   # kRepGatherChunk: output positions per gather step
K_RUN = 1024      # kRepRun: documents of a gather chunk staged in LDS at most


# ------------------------------------------------------------------ reference

class ReplicaRef:
    """rep: the whole packed replica (arrays as long as the totals; tombs always a
    TombBatch, all-zero offsets when no input has tombstones); n_e / n_t: entries /
    tombstones the call writes (the totals, cut at the slot limits); capacity /
    invalid: crdt_ctx_sync reports CRDT_E_CAPACITY / CRDT_E_INVALID."""

    def __init__(self, rep, n_e, n_t, capacity, invalid):
        self.rep, self.n_e, self.n_t, self.capacity, self.invalid = rep, n_e, n_t, capacity, invalid


def _cols(r, kind):
    if kind == "e":
        s = r.state
        return s.offsets, s.counts, s.keys, s.actors, s.counters
    t = r.tombs
    return None if t is None else (t.offsets, t.counts, t.keys, t.actors, t.counters)


def _assemble(sides, side, doc, present, entry_slots, tomb_slots, capacity, invalid):
    """Output document j copies document doc[j] of sides[side[j]] when present[j]."""
    R, n_out = sides[0].state.R, len(doc)
    packed = {}
    for kind in ("e", "t"):
        cnt = np.zeros(n_out, np.int64)
        src = np.zeros(n_out, np.int64)
        for s, r in enumerate(sides):
            c = _cols(r, kind)
            m = present & (side == s)
            if c is None or not m.any():
                continue
            off = np.asarray(c[0], U32).astype(np.int64)
            d = doc[m]
            slots = np.maximum(off[d + 1] - off[d], 0)
            live = slots if c[1] is None else np.asarray(c[1], U32).astype(np.int64)[d]
            capacity |= bool((live > slots).any())
            cnt[m] = np.minimum(live, slots)
            src[m] = off[d]
        o = np.zeros(n_out + 1, np.int64)
        np.cumsum(cnt, out=o[1:])
        total = int(o[-1])
        keys, actors, counters = np.zeros(total, U64), np.zeros(total, U32), np.zeros(total, U64)
        ramp = np.arange(total, dtype=np.int64) - np.repeat(o[:-1], cnt)
        at = np.repeat(src, cnt) + ramp
        sd = np.repeat(side, cnt)
        for s, r in enumerate(sides):
            c = _cols(r, kind)
            m = sd == s
            if c is None or not m.any():
                continue
            keys[m], actors[m], counters[m] = (np.asarray(c[2], U64)[at[m]], np.asarray(c[3], U32)[at[m]],
                                               np.asarray(c[4], U64)[at[m]])
        packed[kind] = ((o % (1 << 32)).astype(U32), cnt.astype(U32), keys, actors, counters, total)
    vv = np.zeros((n_out, R), U64)
    actor = np.zeros(n_out, U32)
    for s, r in enumerate(sides):
        m = present & (side == s)
        if not m.any():
            continue
        vv[m] = np.asarray(r.state.vv, U64)[: r.n_docs * R].reshape(r.n_docs, R)[doc[m]]
        actor[m] = np.asarray(r.doc_actor, U32)[doc[m]] if r.doc_actor is not None else r.actor
    eo, ec, ek, ea, en, te = packed["e"]
    to, tc, tk, ta, tn, tt = packed["t"]
    rep = Replica(AWSetBatch(R, eo, ek, ea, en, vv.reshape(-1), counts=ec), TombBatch(to, tk, ta, tn, counts=tc), 0, actor)
    n_e = te if entry_slots is None else min(te, int(entry_slots))
    n_t = tt if tomb_slots is None else min(tt, int(tomb_slots))
    return ReplicaRef(rep, n_e, n_t, capacity or n_e < te or n_t < tt, invalid)


def replica_select_ref(rep, idx=None, n_idx=None, n_out=None, entry_slots=None, tomb_slots=None):
    """What crdt_replica_select_async writes for a host Replica."""
    n = rep.n_docs
    n_out = n if n_out is None else int(n_out)
    capacity = n_idx is not None and int(n_idx) > n_out
    n_idx = n_out if n_idx is None else min(int(n_idx), n_out)
    doc = np.arange(n_out, dtype=np.int64) if idx is None else np.asarray(idx, U32)[:n_out].astype(np.int64)
    if len(doc) < n_out:
        doc = np.concatenate([doc, np.zeros(n_out - len(doc), np.int64)])
    taken = np.arange(n_out) < n_idx
    bad = taken & (doc >= n)
    present = taken & ~bad
    doc = np.where(present, doc, 0)
    return _assemble([rep], np.zeros(n_out, np.int64), doc, present, entry_slots, tomb_slots, capacity,
                     bool(bad.any()))


def replica_scatter_ref(rep, sub, idx, n_idx=None, entry_slots=None, tomb_slots=None):
    """What crdt_replica_scatter_async writes for host Replicas."""
    assert rep.state.R == sub.state.R
    n, m = rep.n_docs, sub.n_docs
    capacity = n_idx is not None and int(n_idx) > m
    n_idx = m if n_idx is None else min(int(n_idx), m)
    ix = np.asarray(idx, U32)[:n_idx].astype(np.int64)
    ok = ix < n
    js = np.arange(n_idx, dtype=np.int64)[ok]
    invalid = bool((~ok).any()) or len(np.unique(ix[ok])) < len(js)
    inv = np.full(n, -1, np.int64)
    inv[ix[ok][::-1]] = js[::-1]  # written in descending j: the lowest j stays
    side = (inv >= 0).astype(np.int64)
    doc = np.where(inv >= 0, inv, np.arange(n, dtype=np.int64))
    return _assemble([rep, sub], side, doc, np.ones(n, bool), entry_slots, tomb_slots, capacity, invalid)


def same_replica(x, y, tombs=True):
    """Two packed replicas (ref results) are bit-identical; returns the first field that differs."""
    if not same_batch(x.state, y.state):
        return "state"
    if tombs:
        for f in ("offsets", "counts", "keys", "actors", "counters"):
            a, b = np.asarray(getattr(x.tombs, f)), np.asarray(getattr(y.tombs, f))
            if a.shape != b.shape or not (a == b).all():
                return "tombs." + f
    if not (np.asarray(x.doc_actor) == np.asarray(y.doc_actor)).all():
        return "doc_actor"
    return None


# ---------------------------------------------------------------------- cases

def seq_list(start, n, R=2):
    return [(start + 2 * i, i % R, 7 * i + 1) for i in range(n)]


_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def edge_docs():
    """Documents whose packed output has: runs of 2,047, 1, 2,048, 2,049 and 4,097
    (three gather chunks) each followed by a 0- to 3-entry document, so documents
    end at output positions 2,047, 2,048 and 2,049 and later runs start at odd
    positions; 3,000 documents of 0 or 1 entries (more than kRepRun in one
    chunk: the global search); then 300 documents of odd sizes.  The tombstones
    are shorter by the document number mod 3, so the two arrays differ."""
    def make():
        rng = random.Random(9400)
        sizes = []
        for big, small in ((2047, 1), (1, 0), (2048, 3), (2049, 2), (4097, 1)):
            sizes += [big, small]
        sizes += [i % 2 for i in range(3000)] + [rng.choice((1, 3, 5)) for _ in range(300)]
        return [(seq_list(10 * d, m), seq_list(10 * d + 5, max(m - d % 3, 0)), [d + 1, 3]) for d, m in enumerate(sizes)]
    return _once("edge", make)


def big_replica(n=K_PART * K_SCAN + 1, seed=9300):
    """n documents of 0 or 1 entries and 0 or 1 tombstones, one slack slot each, built
    with numpy alone: at the default n, one past 1,024 scan chunks of 1,024."""
    return _once(("big", n, seed), lambda: tiny_replicas(seed, n, 1, R=1, hi=2)[0])


def select_cases():
    """name -> (rep, idx, n_idx, n_out) of every small select case of the GPU file."""
    def make():
        out = {}
        for R in (1, 3, 64):
            _, reps = rand_replicas(9000 + R, 300, 4, R, max_e=9, max_t=4)
            rng = np.random.default_rng(9010 + R)
            for p, r in enumerate(reps):  # layouts: counts NULL / given / slack / stale slack; p == 1: no tombs; odd: doc_actor
                idx = rng.integers(0, 300, 400).astype(U32)  # any order, repeating
                n_idx = (None, 250, 0, 400)[p]
                out["R%d-layout%d" % (R, p)] = (r, idx, n_idx, 400)
        for n in (1, K_SCAN - 1, K_SCAN, K_SCAN + 1):
            out["compact-%d" % n] = (tiny_replicas(9100 + n, n, 1, R=2)[0], None, None, n)
        docs = edge_docs()
        for slack in (0, 1):
            r = make_replica(2, docs, slack=slack, with_counts=True, garbage=np.random.default_rng(9 + slack), actor=1)
            out["edge-compact-slack%d" % slack] = (r, None, None, len(docs))
        perm = np.random.default_rng(9401).permutation(len(docs)).astype(U32)
        out["edge-permuted"] = (make_replica(2, docs, lead=1, actor=1), perm, None, len(docs))
        return out
    return _once("select_cases", make)


def scatter_cases():
    """name -> (rep, sub, idx, n_idx) of every small scatter case of the GPU file."""
    def make():
        out = {}
        for R in (1, 3, 64):
            _, reps = rand_replicas(9500 + R, 300, 4, R, max_e=9, max_t=4)
            _, subs = rand_replicas(9600 + R, 80, 4, R, max_e=12, max_t=6)  # longer, shorter and empty replacements
            rng = np.random.default_rng(9510 + R)
            # (rep, sub): tombs on both, NULL on rep, NULL on sub, NULL on both
            for name, r, s in (("both", reps[0], subs[3]), ("rep-none", reps[1], subs[2]), ("sub-none", reps[3], subs[1]),
                               ("none", reps[1], subs[1])):
                idx = rng.choice(300, 80, replace=False).astype(U32)
                out["R%d-tombs-%s" % (R, name)] = (r, s, idx, None)
            out["R%d-descending" % R] = (reps[2], subs[0], np.arange(299, 219, -1).astype(U32), None)
            out["R%d-n_idx-0" % R] = (reps[2], subs[0], np.arange(80, dtype=U32), 0)
            out["R%d-n_idx-17" % R] = (reps[3], subs[3], rng.choice(300, 80, replace=False).astype(U32), 17)
        for n in (1, K_SCAN - 1, K_SCAN, K_SCAN + 1):
            rep, sub = tiny_replicas(9700 + n, n, 1, R=2)[0], tiny_replicas(9800 + n, (n + 2) // 3, 1, R=2, hi=4)[0]
            idx = np.random.default_rng(n).choice(n, sub.n_docs, replace=False).astype(U32)
            out["scan-%d" % n] = (rep, sub, idx, None)
        docs = edge_docs()
        rng = random.Random(9402)
        sub_docs = rand_docs(rng, 2, 400, max_e=7, max_t=3)
        idx = np.array(rng.sample(range(len(docs)), 400), U32)
        for slack in (0, 1):
            out["edge-slack%d" % slack] = (make_replica(2, docs, slack=slack, with_counts=True, actor=0),
                                           make_replica(2, sub_docs, slack=1 - slack, with_counts=True, actor=1,
                                                        doc_actor=[d % 2 for d in range(400)]), idx, None)
        return out
    return _once("scatter_cases", make)


def big_scatter_case(n=K_PART * K_SCAN + 1, m=5000):
    """(rep, sub, idx) at n documents: m of them replaced, the first and the last among them."""
    def make():
        rep, sub = big_replica(n), tiny_replicas(9301, m, 1, R=1, hi=2)[0]
        rng = np.random.default_rng(9302)
        idx = np.concatenate([[n - 1, 0], rng.choice(np.arange(1, n - 1), m - 2, replace=False)]).astype(U32)
        rng.shuffle(idx)
        return rep, sub, idx
    return _once(("big_scatter", n, m), make)


# --- the rounds ---------------------------------------------------------------

def _op_lists(ops):
    o = np.asarray(ops.op_off, U32)
    return [list(zip(ops.kind[o[d]:o[d + 1]].tolist(), ops.keys[o[d]:o[d + 1]].tolist())) for d in range(ops.n_docs)]


def apply_round_case(seed=9900, n=600, R=3, every=9):
    """(replica, idx, ops of the selected documents, ops of the whole batch with empty
    lists elsewhere): local ops on every 9th document, in descending document order."""
    def make():
        rng = random.Random(seed)
        state, tombs, ops, _ = make_case(rng, n, R, lambda: rng.randint(0, 10), lambda: rng.randint(0, 8))
        actors = np.asarray(ops.doc_actor, U32)
        lists = _op_lists(ops)
        idx = np.arange(n - 1, -1, -every).astype(U32)
        chosen = set(idx.tolist())
        full = OpBatch.from_lists([lists[d] if d in chosen else [] for d in range(n)], actors)
        part = OpBatch.from_lists([lists[d] for d in idx.tolist()], actors[idx])
        return Replica(state, tombs, 0, actors), idx, part, full
    return _once(("apply_round", seed, n, R, every), make)


def delta_round_case(seed=9950, n=3000, R=3, every=23):
    """(a, b, worklist): two replicas (actors 0 and 1) of n documents grown from a
    common ancestor by local Add / Del / AWSetDelta.Del histories (the reference's own
    methods, oracle/awset_ref.py); on every 23rd document one or both sides ran further
    ops, elsewhere both ARE the ancestor.  The worklist is the ascending list of
    documents whose entries, dots, Deleted or clock differ (what digest_diff gives).

    What the generator guarantees: every state is the result of local ops on an
    empty set, so every dot of an entry and of a tombstone is covered by its
    document's own clock.  That is what makes an equal pair a fixed point of both
    AWSetDelta merges (checked in test_sparse_delta_round_is_the_full_exchange): on
    the FULL path the merge of equal states is the state, otherwise no source dot is
    new to the destination clock and every tombstone's dot is already in it."""
    from apply_cases import random_calls, replay

    def make():
        rng = random.Random(seed)
        docs_a, docs_b = [], []
        for d in range(n):
            e, t, vv = [], [], [0] * R
            for actor in ((0, 1, 2) if d % 3 else (0,)):  # a third of the ancestors never saw actor 1: the FULL path
                e, t, vv = replay(actor, R, e, t, vv, random_calls(rng, rng.randint(0, 9), 40, [k for k, _, _ in e]))
            a = b = (e, t, vv)
            if d % every == 5:
                which = rng.choice(("a", "b", "ab"))
                if "a" in which:
                    a = replay(0, R, e, t, vv, random_calls(rng, rng.randint(1, 6), 40, [k for k, _, _ in e]))
                if "b" in which:
                    b = replay(1, R, e, t, vv, random_calls(rng, rng.randint(1, 6), 40, [k for k, _, _ in e]))
            docs_a.append(a)
            docs_b.append(b)
        work = np.array([d for d in range(n) if docs_a[d] != docs_b[d]], U32)
        ra = make_replica(R, docs_a, slack=2, with_counts=True, actor=0)
        rb = make_replica(R, docs_b, slack=1, with_counts=True, actor=1, doc_actor=[1] * n)
        return ra, rb, work, docs_a, docs_b
    return _once(("delta_round", seed, n, R, every), make)


def out_replica(out, like, sel):
    """A merge output (state with counts) as the replica it updates: `sel`'s tombstones and actors."""
    st = AWSetBatch(like.state.R, out.offsets, out.keys, out.actors, out.counters, out.vv, counts=out.counts)
    return Replica(st, sel.tombs, sel.actor, sel.doc_actor)


# ---------------------------------------------------------------------- tests

def test_state_part_is_select_ref_and_scatter_ref():
    for name, (rep, idx, n_idx, n_out) in select_cases().items():
        got = replica_select_ref(rep, idx, n_idx, n_out)
        assert same_batch(got.rep.state, select_ref(rep.state, idx, n_idx, n_out)), name
        assert not got.invalid and not got.capacity
    for name, (rep, sub, idx, n_idx) in scatter_cases().items():
        got = replica_scatter_ref(rep, sub, idx, n_idx)
        assert same_batch(got.rep.state, scatter_ref(rep.state, sub.state, idx, n_idx)), name
        assert not got.invalid and not got.capacity
    # the generators of the 2^20 + 1 document cases, at a size the per-document refs can walk
    rep, sub, idx = big_scatter_case(3000, 500)
    assert same_batch(replica_select_ref(rep).rep.state, select_ref(rep.state))
    assert same_batch(replica_scatter_ref(rep, sub, idx).rep.state, scatter_ref(rep.state, sub.state, idx))
    # reported conditions follow select's and scatter's rules
    r = select_cases()["R3-layout0"][0]
    bad = replica_select_ref(r, np.array([1, 300, 2], U32), 5, 3)
    assert bad.invalid and bad.capacity and bad.rep.state.counts[1] == 0 and bad.rep.doc_actor[1] == 0
    s = scatter_cases()["R3-tombs-both"][1]
    dup = replica_scatter_ref(r, s, np.array([7, 7, 300], U32), 3)
    assert dup.invalid and dup.rep.state.doc(7) == s.state.doc(0) and dup.rep.tombs.doc(7) == s.tombs.doc(0)


def test_tombstones_and_actors_follow_their_documents():
    for name, (rep, idx, n_idx, n_out) in select_cases().items():
        got = replica_select_ref(rep, idx, n_idx, n_out).rep
        lim = n_out if n_idx is None else n_idx
        for j in list(range(0, n_out, 37)) + [n_out - 1]:
            d = int(idx[j]) if idx is not None else j
            want_t = rep.tombs.doc(d) if rep.tombs is not None and j < lim else []
            want_a = (int(rep.doc_actor[d]) if rep.doc_actor is not None else rep.actor) if j < lim else 0
            assert got.tombs.doc(j) == want_t and int(got.doc_actor[j]) == want_a, (name, j)
        assert int(got.tombs.offsets[-1]) == int(got.tombs.counts.astype(np.int64).sum())  # no slack


def test_scatter_of_a_selection_is_the_identity_compacted():
    rng = np.random.default_rng(9020)
    for name, (rep, _, _, _) in select_cases().items():
        want = replica_select_ref(rep).rep
        for idx in (rng.permutation(rep.n_docs)[: rep.n_docs // 3].astype(U32), np.arange(rep.n_docs - 1, -1, -1).astype(U32)):
            sub = replica_select_ref(rep, idx, n_out=len(idx)).rep
            if rep.tombs is None:
                sub = Replica(sub.state, None, 0, sub.doc_actor)
            assert same_replica(replica_scatter_ref(rep, sub, idx).rep, want) is None, name


def test_compaction_of_an_apply_output_is_the_live_tombstones():
    rng = random.Random(9030)
    state, tombs, ops, want = make_case(rng, 200, 3, lambda: rng.randint(0, 8), lambda: rng.randint(0, 8))
    rc, out, tout = oracle.apply(state, ops, tombs)
    assert rc == 0
    slack = np.diff(tout.offsets.astype(np.int64)) - tout.counts
    assert (slack > 0).any()  # apply leaves slack: documents sit at tombs.offsets[d] + op_off[d]
    got = replica_select_ref(Replica(out.as_batch(), tout, 0, ops.doc_actor)).rep
    assert int(got.tombs.offsets[-1]) == int(tout.counts.astype(np.int64).sum())
    for d in range(200):
        assert (got.state.doc(d)[0], got.tombs.doc(d), got.state.doc(d)[1]) == want[d]
        assert int(got.doc_actor[d]) == int(ops.doc_actor[d])


def test_sparse_apply_is_exact():
    """select idx, apply to the sub-replica (C oracle), scatter back == the oracle's apply over
    the whole batch with empty op lists elsewhere, compacted: entries, tombstones, clocks, actors."""
    rep, idx, part, full = apply_round_case()
    rc, out, tout = oracle.apply(rep.state, full, rep.tombs)
    assert rc == 0
    want = replica_select_ref(Replica(out.as_batch(), tout, 0, rep.doc_actor)).rep
    sel = replica_select_ref(rep, idx, n_out=len(idx)).rep
    assert (sel.doc_actor == part.doc_actor).all()  # the selected actors are the ones the ops name
    rc, sout, stout = oracle.apply(sel.state, part, sel.tombs)
    assert rc == 0
    got = replica_scatter_ref(rep, Replica(sout.as_batch(), stout, 0, sel.doc_actor), idx).rep
    assert same_replica(got, want) is None
    assert not same_batch(want.state, replica_select_ref(rep).rep.state)  # the ops changed something


def test_sparse_delta_round_is_the_full_exchange():
    """On delta_round_case's generator (its docstring states what it guarantees): every
    document whose two replicas are equal in entries, dots, Deleted and clock is left
    unchanged, entries and clock, by both AWSetDelta merges; so exchanging only the
    differing documents and scattering them back equals the full exchange, compacted."""
    a, b, work, docs_a, docs_b = delta_round_case()
    n, R = a.n_docs, a.state.R
    assert 0.02 * n < len(work) < 0.06 * n
    for docs in (docs_a, docs_b):  # the guarantee: every dot is covered by its document's clock
        for e, t, vv in docs:
            assert all(c <= vv[x] for _, x, c in e + t)
    full = delta_pair_ref(a, b)
    assert full.rc_ab == 0 and full.rc_ba == 0
    equal = np.ones(n, bool)
    equal[work] = False
    kinds = set()
    for d in np.nonzero(equal)[0].tolist():
        for out, rep in ((full.ab, a), (full.ba, b)):
            o, c = int(out.offsets[d]), int(out.counts[d])
            got = list(zip(out.keys[o:o + c].tolist(), out.actors[o:o + c].tolist(), out.counters[o:o + c].tolist()))
            assert (got, out.vv[d * R:(d + 1) * R].tolist()) == rep.state.doc(d), d
        kinds.add((int(full.kind_ab[d]), int(full.kind_ba[d])))
    assert len({k for k, _ in kinds}) >= 2  # equal pairs on the FULL path and off it
    sa, sb = (replica_select_ref(r, work, n_out=len(work)).rep for r in (a, b))
    part = delta_pair_ref(sa, sb)
    assert part.rc_ab == 0 and part.rc_ba == 0
    for out, sub_out, rep, sel in ((full.ab, part.ab, a, sa), (full.ba, part.ba, b, sb)):
        want = replica_select_ref(out_replica(out, rep, rep)).rep
        got = replica_scatter_ref(rep, out_replica(sub_out, rep, sel), work).rep
        assert same_replica(got, want) is None
    assert not same_batch(replica_select_ref(out_replica(full.ab, a, a)).rep.state, replica_select_ref(a).rep.state)


def test_header_library_and_bindings_have_the_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(abi.HEADER_PATH).read(), flags=re.S)
    go = open(os.path.join(os.path.dirname(PKG), "go", "crdtgpu", "crdtgpu.go")).read()
    for name, n_args, method in (("crdt_replica_select_async", 9, "replica_select_async"),
                                 ("crdt_replica_scatter_async", 9, "replica_scatter_async")):
        assert name in crdtgpu.header_functions()
        assert getattr(abi.lib(), name) is not None  # exported by libcrdtgpu.so
        args = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
        assert len(args.split(",")) == n_args
        assert len(abi.signatures()[name][1]) == n_args and getattr(abi.lib(), name).argtypes is not None
        assert hasattr(crdtgpu.Engine, method) and hasattr(crdtgpu.Engine, method[: -len("_async")])
        assert "C.%s(" % name in go
    fields = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*crdt_replica_out\s*;", text).group(1)
    assert re.findall(r"(\w+)\s*;", fields) == ["state", "tombs", "doc_actor"]
    assert [f for f, _ in abi.CReplicaOut._fields_] == ["state", "tombs", "doc_actor"]
    assert "C.crdt_replica_out{" in go and "func (e *Engine) ReplicaSelect(" in go and "func (e *Engine) ReplicaScatter(" in go
    assert hasattr(crdtgpu, "ReplicaBuffers")


def test_kernel_chunk_constants_are_the_ones_the_gpu_tests_mirror():
    src = open(os.path.join(PKG, "csrc", "replica.hip")).read()

    def const(name):
        expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1)
        for _ in range(4):  # constants defined through earlier ones
            expr = re.sub(r"k\w+", lambda m: "(%s)" % re.search(r"constexpr \w+ %s = ([^;]+);" % m.group(0),
                                                                 src).group(1), expr)
        return eval(expr, {"__builtins__": {}})

    assert const("kRepScanChunk") == K_SCAN and const("kRepPartStep") == K_PART
    assert const("kRepGatherChunk") == K_GATHER and const("kRepRun") == K_RUN
    # the edge cases reach what they are sized for
    eo = replica_select_ref(select_cases()["edge-compact-slack0"][0]).rep.state.offsets.astype(np.int64)
    assert {2047, 2048, 2049} <= set(eo[1:].tolist())  # documents end at these output positions
    assert (np.diff(eo) == 4097).any()  # one document over three chunks
    assert np.bincount(np.minimum(eo[:-1] // K_GATHER, eo[-1] // K_GATHER)).max() > K_RUN  # the global search
    assert (eo[:-1][np.diff(eo) > 1] % 2 == 1).any() and (eo[:-1][np.diff(eo) > 1] % 2 == 0).any()
