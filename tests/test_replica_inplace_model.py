"""CPU: the in-place replica scatter (crdt_replica_scatter_inplace_async) restated
over the resident layout.

replica_scatter_inplace_ref is the expectation of the GPU call
(tests/test_gpu_replica_inplace.py): a vectorised numpy restatement of the contract
in include/crdtgpu.h.  It is pinned here by the call it replaces: compacting its
result and putting the spilled documents back through replica_select_ref /
replica_scatter_ref (tests/test_replica_model.py) equals replica_scatter_ref of the
same arguments, compacted, on every case of tests/replica_inplace_cases.py, on
rand_replicas histories and in the two sparse rounds, against the C oracle.
"""

import os
import re

import numpy as np

import crdtgpu
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch, Replica, TombBatch
from delta_pair_cases import delta_pair_ref
from helpers import PKG
from oracle import oracle
from replica_inplace_cases import K_GATHER, K_PART, K_RUN, K_SCAN, big_case, cases, history_cases
from sources_cases import make_replica
from test_replica_model import (apply_round_case, delta_round_case, out_replica, replica_scatter_ref,
                                replica_select_ref, same_batch)

U32, U64 = np.uint32, np.uint64


# ------------------------------------------------------------------ reference

class InplaceRef:
    """rep: the replica after the call (same layout; arrays copied); spill_j /
    spill_doc: the lists; placed_j / placed_doc: the winners written; capacity /
    invalid: crdt_ctx_sync reports CRDT_E_CAPACITY / CRDT_E_INVALID."""

    def __init__(self, rep, spill_j, spill_doc, placed_j, placed_doc, capacity, invalid):
        self.rep, self.spill_j, self.spill_doc = rep, spill_j, spill_doc
        self.placed_j, self.placed_doc, self.capacity, self.invalid = placed_j, placed_doc, capacity, invalid


def _slots(off):
    o = np.asarray(off, U32).astype(np.int64)
    return np.maximum(o[1:] - o[:-1], 0)


def _move(dst, src, dst_off, src_off, cnt):
    """dst columns [dst_off[i], +cnt[i]) = src columns [src_off[i], +cnt[i])."""
    tot = int(cnt.sum())
    if tot == 0:
        return
    ramp = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    s, d = np.repeat(src_off, cnt) + ramp, np.repeat(dst_off, cnt) + ramp
    for a, b in zip(dst, src):
        a[d] = np.asarray(b)[s]


def replica_scatter_inplace_ref(rep, sub, idx, n_idx=None):
    """What crdt_replica_scatter_inplace_async leaves in a host Replica with counts."""
    assert rep.state.R == sub.state.R and rep.state.counts is not None
    assert sub.tombs is None or rep.tombs is not None
    n, m, R = rep.n_docs, sub.n_docs, rep.state.R
    capacity = n_idx is not None and int(n_idx) > m
    k = m if n_idx is None else min(int(n_idx), m)
    ix = np.asarray(idx, U32)[:k].astype(np.int64)
    ok = ix < n
    js = np.arange(k, dtype=np.int64)[ok]
    invalid = bool((~ok).any()) or len(np.unique(ix[ok])) < len(js)
    inv = np.full(n, -1, np.int64)
    inv[ix[ok][::-1]] = js[::-1]  # written in descending j: the lowest j stays
    win = js[inv[ix[ok]] == js]
    d = ix[win]

    def live(cols):
        if cols is None:
            return np.zeros(len(win), np.int64), np.zeros(len(win), np.int64), False
        slots = _slots(cols.offsets)[win]
        lv = slots if cols.counts is None else np.asarray(cols.counts, U32).astype(np.int64)[win]
        return np.minimum(lv, slots), np.asarray(cols.offsets, U32).astype(np.int64)[win], bool((lv > slots).any())

    ne, so_e, over_e = live(sub.state)
    nt, so_t, over_t = live(sub.tombs)
    ce = _slots(rep.state.offsets)[d]
    ct = _slots(rep.tombs.offsets)[d] if rep.tombs is not None else np.zeros(len(d), np.int64)
    placed = (ne <= ce) & (nt <= ct)
    s = rep.state
    st = AWSetBatch(R, s.offsets, s.keys.copy(), s.actors.copy(), s.counters.copy(), np.asarray(s.vv, U64).copy(),
                    counts=np.asarray(s.counts, U32).copy())
    pj, pd = win[placed], d[placed]
    _move((st.keys, st.actors, st.counters), (sub.state.keys, sub.state.actors, sub.state.counters),
          np.asarray(s.offsets, U32).astype(np.int64)[pd], so_e[placed], ne[placed])
    st.counts[pd] = ne[placed].astype(U32)
    if len(pd):
        st.vv.reshape(-1)[: n * R].reshape(n, R)[pd] = np.asarray(sub.state.vv, U64)[: m * R].reshape(m, R)[pj]
    tb = None
    if rep.tombs is not None:
        t = rep.tombs
        assert t.counts is not None
        tb = TombBatch(t.offsets, t.keys.copy(), t.actors.copy(), t.counters.copy(), counts=np.asarray(t.counts, U32).copy())
        if sub.tombs is not None:
            _move((tb.keys, tb.actors, tb.counters), (sub.tombs.keys, sub.tombs.actors, sub.tombs.counters),
                  np.asarray(t.offsets, U32).astype(np.int64)[pd], so_t[placed], nt[placed])
        tb.counts[pd] = nt[placed].astype(U32)
    da = None
    if rep.doc_actor is not None:
        da = np.asarray(rep.doc_actor, U32).copy()
        da[pd] = np.asarray(sub.doc_actor, U32)[pj] if sub.doc_actor is not None else sub.actor
    return InplaceRef(Replica(st, tb, rep.actor, da), win[~placed].astype(U32), d[~placed].astype(U32), pj, pd,
                      capacity or over_e or over_t, invalid)


def _sel(sub, spill_j):
    got = replica_select_ref(sub, spill_j, n_out=len(spill_j)).rep
    return got if sub.tombs is not None else Replica(got.state, None, 0, got.doc_actor)


def with_fallback(ref, sub):
    """The compaction of ref.rep with the spilled documents put back through the packed calls."""
    if len(ref.spill_j) == 0:
        return replica_select_ref(ref.rep).rep
    return replica_scatter_ref(ref.rep, _sel(sub, ref.spill_j), ref.spill_doc).rep


def same_packed(x, y, actors=True):
    """Two packed replicas (ReplicaRef.rep) are bit-identical; the first field that differs."""
    if not same_batch(x.state, y.state):
        return "state"
    for f in ("offsets", "counts", "keys", "actors", "counters"):
        a, b = np.asarray(getattr(x.tombs, f)), np.asarray(getattr(y.tombs, f))
        if a.shape != b.shape or not (a == b).all():
            return "tombs." + f
    if actors and not (np.asarray(x.doc_actor) == np.asarray(y.doc_actor)).all():
        return "doc_actor"
    return None


def check_contract(rep, sub, idx, n_idx, ref, name):
    """(a) and (c), document by document, from the contract's wording alone."""
    after, R = ref.rep, rep.state.R
    k = sub.n_docs if n_idx is None else min(int(n_idx), sub.n_docs)
    assert (np.diff(ref.spill_j.astype(np.int64)) > 0).all(), name
    assert (ref.spill_doc == np.asarray(idx, U32)[ref.spill_j]).all() and (ref.spill_j < k).all(), name
    assert not set(ref.spill_j.tolist()) & set(ref.placed_j.tolist())
    touched = {("e", int(d)): j for j, d in zip(ref.placed_j.tolist(), ref.placed_doc.tolist())}
    assert len(touched) == len(ref.placed_doc)
    for kind, before, now, src in (("e", rep.state, after.state, sub.state), ("t", rep.tombs, after.tombs, sub.tombs)):
        if before is None:
            assert now is None
            continue
        assert now.offsets is before.offsets
        off = np.asarray(before.offsets, U32).astype(np.int64)
        keep = np.ones(len(before.keys), bool)
        for j, d in zip(ref.placed_j.tolist(), ref.placed_doc.tolist()):
            o = int(off[d])
            if src is None:
                assert int(now.counts[d]) == 0
                continue
            so = int(src.offsets[j])
            slots = int(src.offsets[j + 1]) - so
            ne = min(slots if src.counts is None else int(src.counts[j]), slots)
            assert ne <= int(off[d + 1]) - o and int(now.counts[d]) == ne, (name, kind, j, d)
            keep[o:o + ne] = False
            for f in ("keys", "actors", "counters"):
                assert (getattr(now, f)[o:o + ne] == getattr(src, f)[so:so + ne]).all(), (name, kind, f, j)
        for f in ("keys", "actors", "counters"):
            assert (getattr(now, f)[keep] == getattr(before, f)[keep]).all(), (name, kind, f)
        other = np.ones(rep.n_docs, bool)
        other[ref.placed_doc] = False
        assert (np.asarray(now.counts)[other] == np.asarray(before.counts)[other]).all(), (name, kind)
    other = np.ones(rep.n_docs, bool)
    other[ref.placed_doc] = False
    vb, va = (np.asarray(x.state.vv, U64)[: rep.n_docs * R].reshape(rep.n_docs, R) for x in (rep, after))
    assert (va[other] == vb[other]).all(), name
    assert (va[ref.placed_doc] == np.asarray(sub.state.vv, U64)[: sub.n_docs * R].reshape(sub.n_docs, R)[ref.placed_j]).all()
    if rep.doc_actor is None:
        assert after.doc_actor is None
    else:
        assert (after.doc_actor[other] == np.asarray(rep.doc_actor)[other]).all(), name
        want = np.asarray(sub.doc_actor)[ref.placed_j] if sub.doc_actor is not None else sub.actor
        assert (after.doc_actor[ref.placed_doc] == want).all(), name


def check_equals_packed_scatter(rep, sub, idx, n_idx, ref, name):
    """(b): compaction + fallback == replica_scatter_ref, compacted, bit for bit."""
    want = replica_scatter_ref(rep, sub, idx, n_idx)
    got = with_fallback(ref, sub)
    assert same_packed(got, want.rep, actors=rep.doc_actor is not None) is None, name
    assert (ref.invalid, ref.capacity) == (want.invalid, want.capacity), name


# ---------------------------------------------------------------------- tests

def test_every_case_keeps_the_contract_and_equals_the_packed_scatter():
    for name, (rep, sub, idx, n_idx) in cases().items():
        ref = replica_scatter_inplace_ref(rep, sub, idx, n_idx)
        check_contract(rep, sub, idx, n_idx, ref, name)
        check_equals_packed_scatter(rep, sub, idx, n_idx, ref, name)
    # the generator of the 2^20 + 1 document case, at a size the per-document check can walk
    rep, sub, idx, n_idx = big_case(3 * K_SCAN + 1)
    ref = replica_scatter_inplace_ref(rep, sub, idx, n_idx)
    check_contract(rep, sub, idx, n_idx, ref, "big")
    check_equals_packed_scatter(rep, sub, idx, n_idx, ref, "big")
    assert 0 < len(ref.spill_j) < sub.n_docs


def test_histories():
    """A target that takes one random sub after another, each result the next target."""
    rep, steps = history_cases()
    placed = spilled = 0
    for k, (sub, idx) in enumerate(steps):
        ref = replica_scatter_inplace_ref(rep, sub, idx)
        check_contract(rep, sub, idx, None, ref, k)
        check_equals_packed_scatter(rep, sub, idx, None, ref, k)
        placed, spilled = placed + len(ref.placed_j), spilled + len(ref.spill_j)
        rep = ref.rep
    assert placed and spilled


def test_a_selection_scattered_onto_its_own_replica_changes_nothing():
    """(d): everything is placed, and no live word changes."""
    rng = np.random.default_rng(9021)
    for name in ("R1-tombs-both", "R3-tombs-rep", "R64-tombs-none", "R3-stale", "gather-lead01"):
        rep = cases()[name][0]
        idx = rng.permutation(rep.n_docs)[: rep.n_docs // 2].astype(U32)
        ref = replica_scatter_inplace_ref(rep, _sel(rep, idx), idx)
        assert len(ref.spill_j) == 0 and len(ref.placed_j) == len(idx), name
        for kind in ("state", "tombs"):
            a, b = getattr(ref.rep, kind), getattr(rep, kind)
            for f in ("counts", "keys", "actors", "counters") + (("vv",) if kind == "state" else ()):
                assert a is None or (np.asarray(getattr(a, f)) == np.asarray(getattr(b, f))).all(), (name, kind, f)


def test_census_every_edge_is_reached_by_a_named_case():
    """From the case data alone (no reference): the fit verdicts, replica forms, index
    handling, R, gather edges and spill-scan edges the GPU file relies on."""
    cs = cases()

    def fit(name):
        rep, sub, idx, _ = cs[name]
        eo, to = rep.state.offsets.astype(np.int64), rep.tombs.offsets.astype(np.int64)
        out = []
        for j, d in enumerate(idx.tolist()):
            nt = int(sub.tombs.counts[j]) if sub.tombs is not None else 0
            out.append((int(sub.state.counts[j]), int(eo[d + 1] - eo[d]), nt, int(to[d + 1] - to[d])))
        return out

    f = fit("fit-edges")
    assert any(ne == ce and ne > 0 for ne, ce, _, _ in f) and any(ne == ce + 1 for ne, ce, _, _ in f)
    assert any(ne == 0 and ce > 0 for ne, ce, _, _ in f)
    assert (0, 0, 0, 0) in f and any(ne == 1 and ce == 0 for ne, ce, _, _ in f)
    assert any(ne <= ce and nt > ct for ne, ce, nt, ct in f) and any(ne > ce and nt <= ct for ne, ce, nt, ct in f)
    assert any(nt == ct and nt > 0 and ne <= ce for ne, ce, nt, ct in f)
    for R in (1, 3, 64):
        both, rp, none, stale = (cs["R%d-%s" % (R, k)] for k in ("tombs-both", "tombs-rep", "tombs-none", "stale"))
        assert both[0].state.R == R
        assert both[0].tombs is not None and both[1].tombs is not None and both[1].state.counts is None
        assert both[0].doc_actor is not None and both[1].doc_actor is None  # per document against uniform
        assert rp[0].tombs is not None and rp[1].tombs is None and rp[0].doc_actor is None
        assert none[0].tombs is None and none[1].tombs is None
        for r in stale[:2]:  # stale, non-zero slack on both sides
            o, c = r.state.offsets.astype(np.int64), r.state.counts.astype(np.int64)
            d = int(np.nonzero(o[1:] - o[:-1] > c)[0][0])
            assert r.state.keys[o[d] + c[d]] != 0 and r.doc_actor is not None
    assert cs["dup-low-placed"][2].tolist() == [4, 4, 2] and fit("dup-low-placed")[0][0] <= 3 < fit("dup-low-placed")[1][0]
    assert cs["dup-low-spilled"][2].tolist() == [4, 4, 2] and fit("dup-low-spilled")[1][0] <= 3 < fit("dup-low-spilled")[0][0]
    for k, name in enumerate(("oob-first", "oob-middle", "oob-last")):
        rep, _, idx, _ = cs[name]
        assert [int(x) >= rep.n_docs for x in idx] == [i == k for i in range(3)]
    m = cs["n_idx-0"][1].n_docs
    assert [cs["n_idx-%d" % k][3] for k in (0, 1, 80, 83)] == [0, 1, m, m + 3]
    _, sub, _, _ = cs["sub-count-above-slots"]
    assert (sub.state.counts.astype(np.int64) > np.diff(sub.state.offsets.astype(np.int64))).any()
    assert (sub.tombs.counts.astype(np.int64) > np.diff(sub.tombs.offsets.astype(np.int64))).any()
    # gather edges, in sub's slot space
    par = set()
    for ls in (0, 1):
        for lr in (0, 1):
            rep, sub, idx, _ = cs["gather-lead%d%d" % (ls, lr)]
            so, ro = sub.state.offsets.astype(np.int64), rep.state.offsets.astype(np.int64)
            ends = set((so[1:] - ls).tolist())
            assert {2047, 2048, 2049} <= ends and (np.diff(so) == 4097).any()
            assert np.bincount(np.minimum(so[:-1] // K_GATHER, so[-1] // K_GATHER)).max() > K_RUN  # the global search
            fits = (np.diff(so) >= 2) & (np.diff(so) <= (ro[1:] - ro[:-1])[idx])
            par |= set(zip((so[:-1][fits] % 2).tolist(), (ro[idx.astype(np.int64)][fits] % 2).tolist()))
    assert par == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # spill-scan edges
    for m in (K_SCAN - 1, K_SCAN, K_SCAN + 1):
        want = {"none": 0, "one": 1, "all": m, "alternate": (m + 1) // 2}
        for spill, k in want.items():
            rep, sub, idx, _ = cs["scan-%d-%s" % (m, spill)]
            assert sub.n_docs == m and int((np.diff(rep.state.offsets.astype(np.int64))[idx] == 0).sum()) == k
    rep, sub, idx, _ = big_case()
    assert (sub.n_docs + K_SCAN - 1) // K_SCAN == K_PART + 1
    assert int(np.asarray(sub.state.counts).max()) == 1 and 0 < int((np.diff(rep.state.offsets.astype(np.int64)) == 0).sum())


def test_kernel_chunk_constants_are_the_ones_the_cases_mirror():
    src = open(os.path.join(PKG, "csrc", "replica_inplace.hip")).read()

    def const(name):
        expr = re.search(r"constexpr \w+ %s = ([^;]+);" % name, src).group(1)
        for _ in range(4):  # constants defined through earlier ones
            expr = re.sub(r"k\w+", lambda m: "(%s)" % re.search(r"constexpr \w+ %s = ([^;]+);" % m.group(0),
                                                                 src).group(1), expr)
        return eval(expr, {"__builtins__": {}})

    assert const("kInpScanChunk") == K_SCAN and const("kInpPartStep") == K_PART
    assert const("kInpGatherChunk") == K_GATHER and const("kInpRun") == K_RUN
    mk = open(os.path.join(PKG, "csrc", "Makefile")).read()
    assert all("replica_inplace.hip" in re.search(r"^%s := (.*)$" % v, mk, flags=re.M).group(1) for v in ("SRC", "RU_SRC"))


# --- the rounds -----------------------------------------------------------------

def spare_delta_round(spare_a=2, spare_b=1):
    """delta_round_case's replicas laid out with spare slots after every document."""
    a, b, work, docs_a, docs_b = delta_round_case()
    n = a.n_docs
    ra = make_replica(a.state.R, docs_a, slack=spare_a, with_counts=True, actor=0, doc_actor=[0] * n)
    rb = make_replica(a.state.R, docs_b, slack=spare_b, with_counts=True, actor=1, doc_actor=[1] * n)
    return ra, rb, work


_round = {}


def delta_round_model():
    """(a, b, work, the sub-replicas the sparse exchange produced, the in-place refs,
    the full exchange compacted): computed once, shared with the GPU file."""
    if not _round:
        a, b, work = spare_delta_round()
        full = delta_pair_ref(a, b)
        assert full.rc_ab == 0 and full.rc_ba == 0
        sa, sb = (replica_select_ref(r, work, n_out=len(work)).rep for r in (a, b))
        part = delta_pair_ref(sa, sb)
        assert part.rc_ab == 0 and part.rc_ba == 0
        subs = (out_replica(part.ab, a, sa), out_replica(part.ba, b, sb))
        refs = tuple(replica_scatter_inplace_ref(r, s, work) for r, s in zip((a, b), subs))
        want = tuple(replica_select_ref(out_replica(o, r, r)).rep for o, r in ((full.ab, a), (full.ba, b)))
        _round["delta"] = (a, b, work, subs, refs, want)
    return _round["delta"]


def test_sparse_delta_round_in_place_is_the_full_exchange():
    a, b, work, subs, refs, want = delta_round_model()
    for rep, sub, ref, w in zip((a, b), subs, refs, want):
        assert len(ref.placed_j) >= 1 and len(ref.spill_j) >= 1  # the spare is chosen so that both happen
        assert len(ref.placed_j) + len(ref.spill_j) == len(work)
        check_contract(rep, sub, work, None, ref, "delta")
        assert same_packed(with_fallback(ref, sub), w) is None


def apply_round_model():
    if "apply" not in _round:
        rep, idx, part, full = apply_round_case()
        s, t = rep.state, rep.tombs
        cnt = lambda c: c.counts if c.counts is not None else np.diff(c.offsets.astype(np.int64)).astype(U32)  # noqa: E731
        rep = Replica(AWSetBatch(s.R, s.offsets, s.keys, s.actors, s.counters, s.vv, counts=cnt(s)),
                      TombBatch(t.offsets, t.keys, t.actors, t.counters, counts=cnt(t)), 0, np.asarray(rep.doc_actor, U32))
        rc, out, tout = oracle.apply(rep.state, full, rep.tombs)
        assert rc == 0
        want = replica_select_ref(Replica(out.as_batch(), tout, 0, rep.doc_actor)).rep
        sel = replica_select_ref(rep, idx, n_out=len(idx)).rep
        rc, sout, stout = oracle.apply(sel.state, part, sel.tombs)
        assert rc == 0
        sub = Replica(sout.as_batch(), stout, 0, sel.doc_actor)
        _round["apply"] = (rep, idx, part, sub, replica_scatter_inplace_ref(rep, sub, idx), want)
    return _round["apply"]


def test_sparse_apply_round_in_place_is_the_apply_of_the_whole_batch():
    rep, idx, _, sub, ref, want = apply_round_model()
    check_contract(rep, sub, idx, None, ref, "apply")
    assert len(ref.placed_j) >= 1 and len(ref.placed_j) + len(ref.spill_j) == len(idx)
    assert same_packed(with_fallback(ref, sub), want) is None


# --- the ABI in every layer -----------------------------------------------------

def test_header_library_and_bindings_have_the_entry_point():
    name = "crdt_replica_scatter_inplace_async"
    text = re.sub(r"/\*.*?\*/", "", open(abi.HEADER_PATH).read(), flags=re.S)
    go = open(os.path.join(os.path.dirname(PKG), "go", "crdtgpu", "crdtgpu.go")).read()
    assert name in crdtgpu.header_functions()
    assert getattr(abi.lib(), name) is not None  # exported by libcrdtgpu.so
    args = re.search(name + r"\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(args.split(",")) == 7
    assert len(abi.signatures()[name][1]) == 7 and getattr(abi.lib(), name).argtypes is not None
    for method in ("replica_scatter_inplace_async", "replica_scatter_inplace", "scatter_inplace_async"):
        assert hasattr(crdtgpu.Engine, method)
    assert hasattr(crdtgpu, "SpillBuffers") and hasattr(crdtgpu, "InplaceTarget")
    want = {"crdt_replica_inplace": ["n_docs", "R", "offsets", "counts", "keys", "actors", "counters", "vv", "tomb_offsets",
                                     "tomb_counts", "tkeys", "tactors", "tcounters", "doc_actor"],
            "crdt_spill_out": ["spill_j", "spill_doc", "n_spill"]}
    for (st, fields), c in zip(want.items(), (abi.CReplicaInplace, abi.CSpillOut)):
        body = re.search(r"typedef\s+struct\s*\{([^{}]*)\}\s*%s\s*;" % st, text).group(1)
        assert re.findall(r"(\w+)\s*;", body) == fields
        assert [f for f, _ in c._fields_] == fields
        lit = re.search(r"C\.%s\{(.*?)\}" % st, go, flags=re.S).group(1)
        assert set(re.findall(r"(\w+):", lit)) <= set(fields) and "C.%s{" % st in go
    assert "func (e *Engine) ReplicaScatterInPlace(" in go and "C.%s(" % name in go
    call = re.search(r"C\.%s\((.*?)\);" % name, go, flags=re.S).group(1)
    depth, n = 0, 1
    for ch in call:
        depth += ch in "([{"
        depth -= ch in ")]}"
        n += ch == "," and depth == 0
    assert n == 7
    assert "crdt_replica_scatter_async" in re.search(r"/\* ---- in-place replica scatter.*?\*/", open(abi.HEADER_PATH).read(),
                                                     flags=re.S).group(0)  # the contract cites what it replaces
