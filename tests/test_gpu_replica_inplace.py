"""GPU: crdt_replica_scatter_inplace_async (csrc/replica_inplace.hip) against
replica_scatter_inplace_ref (tests/test_replica_inplace_model.py), bit-exact.

Every written array of the target sits between two guard zones of poison (words
all-ones) inside a larger allocation.  After a call the guards must still hold
poison and the array must equal the reference's, which keeps every word the
contract calls untouched as it was: the other documents, the slack of the placed
ones, stale values included.  The spill lists are poisoned too, so the words at
or past *n_spill must still hold poison.  The cases, and the kernel units they
are sized around, are those of tests/replica_inplace_cases.py.
"""

import ctypes

import numpy as np
import pytest

import crdtgpu
from crdtgpu import CRDT_E_CAPACITY, CRDT_E_INVALID, CRDT_E_WORKSPACE, abi
from crdtgpu.batch import (AWSetBatch, CompareBuffers, InplaceTarget, OutBuffers, Replica, ReplicaBuffers, SpillBuffers,
                           TombBatch, TombBuffers, _np)
from replica_inplace_cases import K_PART, K_SCAN, big_case, cases
from test_gpu_compare import _code, dev_of
from test_gpu_replica import assert_replica, poisoned, word, words
from test_replica_inplace_model import apply_round_model, delta_round_model, replica_scatter_inplace_ref
from test_replica_model import ReplicaRef

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
GUARD = 16  # elements: 64 B of u32, 128 B of u64, so a guarded array keeps its 16 B alignment
STATE = ("counts", "keys", "actors", "counters", "vv")


@pytest.fixture(scope="module")
def torch():
    import torch as t

    assert t.cuda.is_available(), "GPU tests need a HIP device"
    return t


@pytest.fixture(scope="module")
def eng(torch):
    e = crdtgpu.Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------- helpers

def guarded(torch, a, lead=GUARD):
    """(view holding a, the allocation around it): `lead` poisoned elements before and GUARD after."""
    a = np.ascontiguousarray(a)
    dt = torch.int32 if a.dtype.itemsize == 4 else torch.int64
    big = torch.full((lead + len(a) + GUARD,), -1, dtype=dt, device=dev_of(torch))
    view = big[lead:lead + max(len(a), 1)]  # (never empty: an empty tensor has no address)
    if len(a):
        view[: len(a)].copy_(torch.from_numpy(a.view(np.int32 if a.dtype.itemsize == 4 else np.int64).copy()))
    return view, big


class Target:
    """A host Replica uploaded as an in-place target with every written array guarded."""

    def __init__(self, torch, rep, lead=GUARD):
        dev = dev_of(torch)
        self.lead, self.bigs = lead, {}
        s, t = rep.state, rep.tombs

        def g(name, a):
            view, big = guarded(torch, a, lead)
            self.bigs[name] = big
            return view

        st = AWSetBatch(s.R, words(torch, s.offsets), g("state.keys", s.keys), g("state.actors", s.actors),
                        g("state.counters", s.counters), g("state.vv", s.vv), counts=g("state.counts", s.counts))
        tb = None
        if t is not None:
            tb = TombBatch(words(torch, t.offsets), g("tombs.keys", t.keys), g("tombs.actors", t.actors),
                           g("tombs.counters", t.counters), counts=g("tombs.counts", t.counts))
        da = g("doc_actor", rep.doc_actor) if rep.doc_actor is not None else None
        self.offsets = (st.offsets.clone(), None if tb is None else tb.offsets.clone())
        self.rep = Replica(st, tb, rep.actor, da)
        self.target = InplaceTarget.of(self.rep)
        assert dev is not None

    def check(self, torch, want):
        """Guards still poison; every array equals `want` (a host Replica of the same layout)."""
        for name, big in self.bigs.items():
            holder, f = (want, "doc_actor") if name == "doc_actor" else (getattr(want, name.split(".")[0]), name.split(".")[1])
            exp = np.ascontiguousarray(getattr(holder, f))
            got = _np(big, U32 if exp.dtype.itemsize == 4 else U64)
            ones = np.iinfo(got.dtype).max
            assert (got[: self.lead] == ones).all() and (got[self.lead + len(exp):] == ones).all(), name + ": guard written"
            body = got[self.lead:self.lead + len(exp)]
            if not (body == exp).all():
                i = int(np.nonzero(body != exp)[0][0])
                raise AssertionError("%s differs first at %d of %d: gpu %d, expected %d" % (name, i, len(exp), body[i], exp[i]))
        assert torch.equal(self.rep.state.offsets, self.offsets[0]), "offsets written"
        if self.rep.tombs is not None:
            assert torch.equal(self.rep.tombs.offsets, self.offsets[1]), "tomb offsets written"


def spill_buffers(torch, n_sub):
    sp = SpillBuffers(n_sub, device=dev_of(torch))
    for t in (sp.spill_j, sp.spill_doc, sp.n_spill):
        t.fill_(-1)
    return sp


def check_spill(sp, ref):
    k = len(ref.spill_j)
    assert int(_np(sp.n_spill, U32)[0]) == k, "n_spill"
    for f in ("spill_j", "spill_doc"):
        got = _np(getattr(sp, f), U32)
        assert (got[:k] == getattr(ref, f)).all(), f
        assert (got[k:] == 2 ** 32 - 1).all(), f + " written at or past n_spill"


def expect_code(eng, ref):
    if ref.invalid:
        assert _code(eng.sync) == CRDT_E_INVALID
    elif ref.capacity:
        assert _code(eng.sync) == CRDT_E_CAPACITY
    else:
        eng.sync()


def run_case(eng, torch, rep, sub, idx, n_idx, lead=GUARD, dev_sub=None, stream=None):
    """(Target, spill buffers, ref) after one call; not synced."""
    ref = replica_scatter_inplace_ref(rep, sub, idx, n_idx)
    tgt = Target(torch, rep, lead)
    sp = spill_buffers(torch, sub.n_docs)
    eng.replica_scatter_inplace_async(tgt.target, dev_sub or sub.to(dev_of(torch)), words(torch, idx), sp,
                                      word(torch, n_idx), stream=stream)
    return tgt, sp, ref


def shifted(torch, t):
    """The same values in a tensor whose first element sits one element past an aligned address."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    big[1:].copy_(t)
    return big[1:]


# ------------------------------------------------- 1. the case table

@pytest.mark.parametrize("name", sorted(cases()))
def test_cases(eng, torch, name):
    """Fit verdicts (ne == ce, ce + 1, 0; zero capacity; entries fit and tombstones do
    not, and the reverse), replica forms (tombstones on both sides, on rep only, on
    neither; doc_actor against a uniform actor; counts NULL on sub; stale slack), index
    handling (duplicates, out of range, *n_idx 0 / 1 / m / above m, a sub count above its
    slots), R 1 / 3 / 64, the gather edges and the spill-scan edges: placed prefixes,
    counts, clocks, actors, spill lists, *n_spill and the reported code are the
    reference's; the guards and every untouched word are as before."""
    rep, sub, idx, n_idx = cases()[name]
    tgt, sp, ref = run_case(eng, torch, rep, sub, idx, n_idx)
    expect_code(eng, ref)
    tgt.check(torch, ref.rep)
    check_spill(sp, ref)


def test_partials_scan_steps(eng, torch):
    """1,048,577 sub documents of 0 or 1 entries: 1,025 partial sums, so the partials scan
    takes a second step; a third of the targets have no entry slot."""
    rep, sub, idx, n_idx = big_case()
    assert (sub.n_docs + K_SCAN - 1) // K_SCAN == K_PART + 1
    tgt, sp, ref = run_case(eng, torch, rep, sub, idx, n_idx)
    expect_code(eng, ref)
    tgt.check(torch, ref.rep)
    check_spill(sp, ref)
    assert 0 < len(ref.spill_j) < sub.n_docs


# ------------------------------------------------------ 2. pair alignment

@pytest.mark.parametrize("where", ["inputs", "target", "both"])
def test_unaligned_columns_give_the_same_bits(eng, torch, where):
    """Columns one element off their alignment (4 B for the actors, 8 B for keys and
    counters): that side goes element by element, and every bit is the same."""
    rep, sub, idx, n_idx = cases()["gather-lead10"]
    ds = sub.to(dev_of(torch))
    if where != "target":
        for cols in (ds.state, ds.tombs):
            for f in ("keys", "actors", "counters"):
                setattr(cols, f, shifted(torch, getattr(cols, f)))
                assert getattr(cols, f).data_ptr() % (8 if f == "actors" else 16) != 0
    lead = GUARD + 1 if where != "inputs" else GUARD
    tgt, sp, ref = run_case(eng, torch, rep, sub, idx, n_idx, lead=lead, dev_sub=ds)
    if where != "inputs":
        assert tgt.rep.state.keys.data_ptr() % 16 != 0 and tgt.rep.tombs.actors.data_ptr() % 8 != 0
    expect_code(eng, ref)
    tgt.check(torch, ref.rep)
    check_spill(sp, ref)


# ------------------------------------------------------ 3. the state-only wrapper

def test_state_only_wrapper(eng, torch):
    """scatter_inplace_async (no tombstones, no actors) writes what the replica form writes
    for the state, and leaves tombstones and actors alone."""
    for name in ("R3-tombs-none", "R64-tombs-none", "scan-1025-alternate"):
        rep, sub, idx, n_idx = cases()[name]
        bare = Replica(rep.state, None, rep.actor, None)
        ref = replica_scatter_inplace_ref(bare, Replica(sub.state), idx, n_idx)
        tgt = Target(torch, rep)
        sp = spill_buffers(torch, sub.n_docs)
        eng.scatter_inplace_async(tgt.rep.state, sub.state.to(dev_of(torch)), words(torch, idx), sp, word(torch, n_idx))
        expect_code(eng, ref)
        tgt.check(torch, Replica(ref.rep.state, rep.tombs, rep.actor, rep.doc_actor))
        check_spill(sp, ref)
        if rep.tombs is None:  # the replica form of the same arguments: the same state, bit for bit
            full = replica_scatter_inplace_ref(rep, sub, idx, n_idx)
            assert all((np.asarray(getattr(full.rep.state, f)) == np.asarray(getattr(ref.rep.state, f))).all() for f in STATE)


# ---------------------------------------------------------------- 4. errors

def test_invalid_arguments(eng, torch):
    """What the call itself returns CRDT_E_INVALID for; nothing is launched."""
    dev = dev_of(torch)
    rep, sub, idx, _ = cases()["R3-tombs-both"]
    other = cases()["R1-tombs-both"][1]
    tgt = Target(torch, rep)
    ds, didx = sub.to(dev), words(torch, idx)
    sp = spill_buffers(torch, sub.n_docs)
    lib, ctx = abi.lib(), eng._ctx
    good_t, cs, cp = tgt.target.c(), ds.c(), sp.c()

    def call(t=good_t, s=cs, i=didx.data_ptr(), p=cp, c=ctx):
        by = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
        return lib.crdt_replica_scatter_inplace_async(c, by(t), by(s), i, None, by(p), None)

    def target(**kw):
        t = tgt.target.c()
        for k, v in kw.items():
            setattr(t, k, v)
        return t

    assert call(c=None) == call(t=None) == call(s=None) == call(i=None) == call(p=None) == CRDT_E_INVALID
    for f in ("offsets", "counts", "keys", "actors", "counters", "vv", "tomb_counts", "tkeys"):
        assert call(t=target(**{f: None})) == CRDT_E_INVALID, f
    assert call(t=target(R=2)) == call(t=target(R=0)) == CRDT_E_INVALID  # R differs from sub's, or out of range
    assert call(s=other.to(dev).c()) == CRDT_E_INVALID
    wide = abi.CAWSetBatch(sub.n_docs, 65, *[getattr(cs._keep[0], f) for f in ("offsets", "counts", "keys", "actors",
                                                                             "counters", "vv")])
    assert call(t=target(R=65), s=abi.CReplica(ctypes.addressof(wide), None, None, 0)) == CRDT_E_INVALID
    assert call(t=target(tomb_offsets=None)) == CRDT_E_INVALID  # sub has tombstones, the replica keeps none
    t = ds.tombs
    assert call(s=Replica(ds.state, TombBatch(None, t.keys, t.actors, t.counters), 0).c()) == CRDT_E_INVALID
    for f in ("spill_j", "spill_doc", "n_spill"):
        bad = sp.c()
        setattr(bad, f, None)
        assert call(p=bad) == CRDT_E_INVALID, f
    # a written array of rep starting where an array of the same kind of sub starts
    for f, src in (("counts", ds.state.offsets), ("keys", ds.state.keys), ("vv", ds.state.vv), ("actors", ds.state.actors),
                   ("tkeys", ds.tombs.counters), ("tomb_counts", ds.tombs.offsets), ("doc_actor", ds.state.actors)):
        assert call(t=target(**{f: src.data_ptr()})) == CRDT_E_INVALID, f
    eng.sync()
    tgt.check(torch, rep)
    assert all(bool((x == -1).all()) for x in (sp.spill_j, sp.spill_doc, sp.n_spill))


def test_empty_calls(eng, torch):
    """n_docs == 0 or no sub documents: *n_spill = 0 and nothing else."""
    dev = dev_of(torch)
    rep, sub, idx, _ = cases()["R3-tombs-both"]
    z32, z64 = np.zeros(0, U32), np.zeros(0, U64)
    none = Replica(AWSetBatch(3, np.zeros(1, U32), z64, z32, z64, z64, counts=z32),
                   TombBatch(np.zeros(1, U32), z64, z32, z64, counts=z32), 1)
    for r, s in ((rep, none), (none, sub), (none, none)):
        tgt = Target(torch, r)
        sp = spill_buffers(torch, max(s.n_docs, 1))
        eng.replica_scatter_inplace_async(tgt.target, s.to(dev), words(torch, idx), sp)
        eng.sync()
        tgt.check(torch, r)
        assert int(_np(sp.n_spill, U32)[0]) == 0
        assert bool((sp.spill_j == -1).all()) and bool((sp.spill_doc == -1).all())


# ------------------------------------------------ 5. determinism, capture, streams

def test_run_to_run_identity(eng, torch):
    """No atomic decides a position: two runs give the same bits, spill lists included."""
    rep, sub, idx, n_idx = cases()["gather-lead11"]
    runs = []
    for _ in range(2):
        tgt, sp, ref = run_case(eng, torch, rep, sub, idx, n_idx)
        eng.sync()
        runs.append((tgt, sp))
    (t0, s0), (t1, s1) = runs
    for name in t0.bigs:
        assert torch.equal(t0.bigs[name], t1.bigs[name]), name
    for f in ("spill_j", "spill_doc", "n_spill"):
        assert torch.equal(getattr(s0, f), getattr(s1, f)), f


def test_graph_capture(torch):
    """Captured on a reserved context and replayed with idx and *n_idx changed in between, the
    call equals the eager one; on an unreserved context (more than 1,024 documents) the capture
    is refused with CRDT_E_WORKSPACE and launches nothing."""
    dev = dev_of(torch)
    rep, sub, idx, _ = cases()["scan-1025-alternate"]
    m = sub.n_docs
    e = crdtgpu.Engine(0)
    try:
        ds = sub.to(dev)
        idxd = torch.zeros(m, dtype=torch.int32, device=dev)
        nd = torch.zeros(1, dtype=torch.int32, device=dev)
        tgt = Target(torch, rep)
        sp = spill_buffers(torch, m)
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.replica_scatter_inplace_async(tgt.target, ds, idxd, sp, nd, stream=torch.cuda.current_stream())
        assert ei.value.code == CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        tgt.check(torch, rep)
        assert bool((sp.n_spill == -1).all())
        e.reserve(rep.n_docs)
        tgt = Target(torch, rep)
        ct, cs, cp = tgt.target.c(), ds.c(), sp.c()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.replica_scatter_inplace_async(ct, cs, idxd, cp, nd, stream=torch.cuda.current_stream())
        now = rep
        for ix, k in ((idx, m), (np.roll(idx, 3), 100), (idx, 0)):
            idxd.copy_(words(torch, ix))
            nd.fill_(k)
            for t in (sp.spill_j, sp.spill_doc, sp.n_spill):
                t.fill_(-1)
            g.replay()
            e.sync(torch.cuda.current_stream())
            ref = replica_scatter_inplace_ref(now, sub, ix, k)
            tgt.check(torch, ref.rep)
            check_spill(sp, ref)
            now = ref.rep  # the target keeps what the replay before wrote
    finally:
        e.close()


def test_ordering_across_two_streams(eng, torch):
    """Two calls on two streams share the context's workspace: the second is ordered after the first."""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []
    for name, s in (("gather-lead00", s1), ("scan-1025-one", s2), ("R64-stale", s1)):
        rep, sub, idx, n_idx = cases()[name]
        with torch.cuda.stream(s):
            got.append(run_case(eng, torch, rep, sub, idx, n_idx, stream=s))
    eng.sync(s1)
    eng.sync(s2)
    for tgt, sp, ref in got:
        tgt.check(torch, ref.rep)
        check_spill(sp, ref)


# ---------------------------------------------------------------- 6. rounds

def fallback(eng, torch, tgt_rep, host_rep, sub, sp, m, R, e_slots, t_slots):
    """The spilled documents through the packed calls, driven by the spill lists on the device."""
    sel = ReplicaBuffers(m, R, e_slots, t_slots, device=dev_of(torch))
    eng.replica_select_async(sub, sel, sp.spill_j, sp.n_spill, m)
    out = poisoned(torch, host_rep.n_docs, R, int(host_rep.state.offsets[-1]) + e_slots,
                   int(host_rep.tombs.offsets[-1]) + t_slots)
    eng.replica_scatter_async(tgt_rep, sel.as_replica(), sp.spill_doc, out, sp.n_spill)
    return out


def as_ref(want):
    return ReplicaRef(want, int(want.state.offsets[-1]), int(want.tombs.offsets[-1]), False, False)


def test_sparse_delta_round_in_place(eng, torch):
    """digest x 2, digest_diff, replica_select x 2, delta_exchange, the in-place scatter x 2 with
    the delta-exchange outputs as sub as they stand, then the fallback for what spilled, nothing
    downloaded in between: the compacted result is the full exchange's (the model's answer)."""
    dev = dev_of(torch)
    a, b, work, subs, refs, want = delta_round_model()
    n, R, m = a.n_docs, a.state.R, 256
    assert len(work) <= m
    da, db = a.to(dev), b.to(dev)
    dig_a = torch.empty(2 * n, dtype=torch.int64, device=dev)
    dig_b = torch.empty(2 * n, dtype=torch.int64, device=dev)
    eng.digest_async(da.state, dig_a, da.tombs)
    eng.digest_async(db.state, dig_b, db.tombs)
    cmp = CompareBuffers(n, device=dev)
    eng.digest_diff_async(dig_a, dig_b, n, cmp)
    sa, sb = (ReplicaBuffers(m, R, 40 * m, 40 * m, device=dev) for _ in range(2))
    eng.replica_select_async(da, sa, cmp.worklist, cmp.n_work, m)
    eng.replica_select_async(db, sb, cmp.worklist, cmp.n_work, m)
    yab, yba = (OutBuffers(m, R, 80 * m, device=dev) for _ in range(2))
    eng.delta_exchange_async(sa.as_replica(), sb.as_replica(), yab, yba)
    outs = []
    for d, h, y, s in ((da, a, yab, sa), (db, b, yba, sb)):
        sub = Replica(y.as_batch(), s.tombs, 0, s.doc_actor)
        sp = spill_buffers(torch, m)
        eng.replica_scatter_inplace_async(d, sub, cmp.worklist, sp, cmp.n_work)
        outs.append((sp, fallback(eng, torch, d, h, sub, sp, m, R, 80 * m, 40 * m)))
    eng.sync()
    assert (cmp.numpy()[2] == work).all()
    for (sp, out), ref, w in zip(outs, refs, want):
        check_spill(sp, ref)
        out.entry_slots, out.tomb_slots = out.state.keys.numel(), out.tombs.keys.numel()
        assert_replica(out, as_ref(w))


def test_sparse_apply_round_in_place(eng, torch):
    """replica_select, apply, the in-place scatter with the apply output as sub as it stands
    (tombstones at tombs.offsets[d] + op_off[d]), then the fallback: the compacted result is
    the oracle's apply of the whole batch."""
    dev = dev_of(torch)
    rep, idx, part, _, ref, want = apply_round_model()
    n, R, m = rep.n_docs, rep.state.R, len(idx)
    dr, didx = rep.to(dev), words(torch, idx)
    e_sel, t_sel = int(rep.state.offsets[-1]), int(rep.tombs.offsets[-1])
    sel = ReplicaBuffers(m, R, e_sel, t_sel, device=dev)
    eng.replica_select_async(dr, sel, didx, None, m)
    pops = int(part.op_off[-1])
    so = OutBuffers(m, R, e_sel + pops, device=dev)
    st = TombBuffers(m, t_sel + pops, device=dev)
    dpart = part.to(dev)
    dpart.doc_actor = sel.doc_actor
    eng.apply_async(sel.state.as_batch(), dpart, so, sel.tombs, st)
    sub = Replica(so.as_batch(), st, 0, sel.doc_actor)
    sp = spill_buffers(torch, m)
    eng.replica_scatter_inplace_async(dr, sub, didx, sp)
    out = fallback(eng, torch, dr, rep, sub, sp, m, R, e_sel + pops, t_sel + pops)
    eng.sync()
    check_spill(sp, ref)
    out.entry_slots, out.tomb_slots = out.state.keys.numel(), out.tombs.keys.numel()
    assert_replica(out, as_ref(want))
