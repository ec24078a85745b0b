"""GPU: crdt_replica_repack_async (csrc/replica_repack.hip) against
replica_repack_ref (tests/test_replica_repack_model.py) on every case of
tests/replica_repack_cases.py.  Every call writes into over-allocated outputs
filled with all-ones words, and every word outside a live prefix must still be
all-ones afterwards: the layout's slack is never written.  Offsets, counts,
clocks, actors and the reported code are the reference's, bit for bit.
"""

import ctypes

import numpy as np
import pytest

import crdtgpu
from crdtgpu import CRDT_E_CAPACITY, CRDT_E_INVALID, CRDT_E_WORKSPACE, abi
from crdtgpu.batch import (AWSetBatch, CompareBuffers, Headroom, InplaceTarget, OutBuffers, Replica, ReplicaBuffers,
                           TombBatch, TombBuffers, _np, repack_slots)
from replica_repack_cases import K_PART, K_SCAN, ONES32, ROUND_ROOM, big_case, cases
from test_gpu_compare import _code, dev_of
from test_gpu_replica import assert_replica, poisoned, repoison, shifted, word, words
from test_gpu_replica_inplace import as_ref, spill_buffers
from test_replica_repack_model import (apply_round_model, case_ref, delta_round_model, ref_of, replica_repack_ref,
                                       room_of)

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
MAXK = 2 ** 64 - 1
SPARE = 5  # slots allocated past the limits the call is given


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

def limits(c, ref):
    """The slot limits a case's call is given (exactly the capacity totals when the case names none)."""
    es = ref.total["e"] if c.entry_slots is None else c.entry_slots
    ts = ref.total["t"] if c.tomb_slots is None else c.tomb_slots
    return es, ts


def launch(eng, torch, c, ref, out=None, dev_rep=None, dev_sub=None, stream=None):
    """One call of case c into poisoned outputs (out->tombs always passed); not synced."""
    es, ts = limits(c, ref)
    if out is None:
        out = poisoned(torch, c.n_out, c.rep.state.R, es + SPARE, ts + SPARE)
    out.entry_slots, out.tomb_slots = es, ts
    dev = dev_of(torch)
    eng.replica_repack_async(dev_rep or c.rep.to(dev), out, dev_sub or (c.sub.to(dev) if c.sub is not None else None),
                             words(torch, c.idx), word(torch, c.n_idx), c.n_out, room_of(c.er), room_of(c.tr),
                             stream=stream)
    return out


def assert_repack(out, ref):
    """A poisoned output equals ref: offsets, counts, clocks and actors word for word,
    the live prefixes below the limits, and all-ones in every other slot."""
    n, R = out.n_docs, out.R
    st, tb = out.state, out.tombs
    assert (_np(st.offsets, U32)[: n + 1] == ref.off["e"]).all(), "offsets"
    assert (_np(st.counts, U32)[:n] == ref.cnt["e"]).all(), "counts"
    assert (_np(st.vv, U64)[: n * R] == ref.vv).all(), "vv"
    assert (_np(out.doc_actor, U32)[:n] == ref.doc_actor).all(), "doc_actor"
    assert (_np(tb.offsets, U32)[: n + 1] == ref.off["t"]).all(), "tomb offsets"
    assert (_np(tb.counts, U32)[:n] == ref.cnt["t"]).all(), "tomb counts"
    for kind, got in (("e", st), ("t", tb)):
        want = ref.columns(kind, got.keys.numel(), fill=MAXK)
        for f, w in zip(("keys", "actors", "counters"), want):
            g = _np(getattr(got, f), U32 if f == "actors" else U64)
            if not (g == w[: len(g)]).all():
                i = int(np.nonzero(g != w[: len(g)])[0][0])
                raise AssertionError("%s %s differs first at %d: gpu %d, expected %d" % (kind, f, i, g[i], w[i]))


def expect_code(eng, ref, stream=None):
    if ref.invalid:
        assert _code(lambda: eng.sync(stream)) == CRDT_E_INVALID
    elif ref.capacity:
        assert _code(lambda: eng.sync(stream)) == CRDT_E_CAPACITY
    else:
        eng.sync(stream)


def tensors(out):
    return [out.state.offsets, out.state.counts, out.state.keys, out.state.actors, out.state.counters, out.state.vv,
            out.tombs.offsets, out.tombs.counts, out.tombs.keys, out.tombs.actors, out.tombs.counters, out.doc_actor]


# ------------------------------------------------- 1. the case table

@pytest.mark.parametrize("name", sorted(cases()))
def test_cases(eng, torch, name):
    """Policy edges, every select and scatter form, the scan and gather edges and the
    capacity edges (tests/test_replica_repack_model.py's census names them)."""
    c, ref = cases()[name], case_ref(name)
    out = launch(eng, torch, c, ref)
    expect_code(eng, ref)
    assert_repack(out, ref)


def test_partials_scan_steps(eng, torch):
    """2^20 + 1 documents of at most one entry: 1,025 partial sums, a second partials step."""
    c, ref = big_case(), case_ref("big")
    assert (c.n_out + K_SCAN - 1) // K_SCAN == K_PART + 1
    out = launch(eng, torch, c, ref)
    expect_code(eng, ref)
    assert_repack(out, ref)


# ------------------------------------------------- 2. both policies NULL

@pytest.mark.parametrize("name", ["pol-both-null", "sel-R3-layout3", "sel-edge-compact-slack1", "sct-R64-tombs-both",
                                  "sct-edge-slack0", "sct-scan-1025"])
def test_both_policies_null_is_select_and_scatter(eng, torch, name):
    """The same inputs through crdt_replica_select_async / crdt_replica_scatter_async: equal bits in every array."""
    c = cases()[name]._replace(er=None, tr=None)
    ref = ref_of(c)
    out = launch(eng, torch, c, ref)
    old = poisoned(torch, c.n_out, c.rep.state.R, ref.total["e"] + SPARE, ref.total["t"] + SPARE)
    old.entry_slots, old.tomb_slots = limits(c, ref)
    dev = dev_of(torch)
    if c.sub is None:
        eng.replica_select_async(c.rep.to(dev), old, words(torch, c.idx), word(torch, c.n_idx), c.n_out)
    else:
        eng.replica_scatter_async(c.rep.to(dev), c.sub.to(dev), words(torch, c.idx), old, word(torch, c.n_idx))
    eng.sync()
    for a, b in zip(tensors(out), tensors(old)):
        assert torch.equal(a, b)
    if c.rep.tombs is None and (c.sub is None or c.sub.tombs is None):
        old.tombs.keys = old.tombs.actors = old.tombs.counters = None
    assert_replica(old, ref.packed)


# ------------------------------------------------- 3. alignment

@pytest.mark.parametrize("where", ["inputs", "outputs", "both"])
def test_unaligned_columns_give_the_same_bits(eng, torch, where):
    """Columns one element past a 16 B boundary, on the inputs, the outputs or both: the element-wise paths."""
    dev = dev_of(torch)
    for name in ("gather-doubling", "gather-odd-starts", "sct-edge-slack1"):
        c, ref = cases()[name], case_ref(name)
        dr, ds = c.rep.to(dev), c.sub.to(dev) if c.sub is not None else None
        es, ts = limits(c, ref)
        out = poisoned(torch, c.n_out, c.rep.state.R, es + SPARE, ts + SPARE)
        if where != "outputs":
            for r in (dr, ds):
                for b in (r.state, r.tombs) if r is not None else ():
                    for f in ("keys", "actors", "counters"):
                        setattr(b, f, shifted(torch, getattr(b, f)))
        if where != "inputs":
            for b in (out.state, out.tombs):
                for f in ("keys", "actors", "counters"):
                    setattr(b, f, shifted(torch, getattr(b, f)))
                    assert getattr(b, f).data_ptr() % 16 != 0
        launch(eng, torch, c, ref, out=out, dev_rep=dr, dev_sub=ds)
        expect_code(eng, ref)
        assert_repack(out, ref)


# ------------------------------------------------- 4. returned errors, empty calls

def test_invalid_arguments(eng, torch):
    """What the call itself returns CRDT_E_INVALID for; nothing is launched."""
    dev = dev_of(torch)
    c = cases()["sct-R3-tombs-both"]
    other = cases()["sct-R1-tombs-both"].sub
    dr, ds, didx = c.rep.to(dev), c.sub.to(dev), words(torch, c.idx)
    n = c.rep.n_docs
    out = poisoned(torch, n, 3, 20000, 5000)
    lib, ctx = abi.lib(), eng._ctx
    cr, cs, co = dr.c(), ds.c(), out.c()
    good = abi.CHeadroom(1, 1, 0, 2)

    def call(r=cr, s=None, i=None, n_out=n, er=good, tr=good, o=co, cx=ctx):
        ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
        return lib.crdt_replica_repack_async(cx, ref(r), ref(s), i, None, n_out, ref(er), ref(tr), 20000, 5000, ref(o),
                                             None)

    for align in (0, 3, 6, 128, 2 ** 31):
        assert call(er=abi.CHeadroom(0, 0, 0, align)) == call(tr=abi.CHeadroom(0, 0, 0, align)) == CRDT_E_INVALID, align
    assert call(er=abi.CHeadroom(0, 1, 32, 1)) == call(tr=abi.CHeadroom(0, 1, 40, 1)) == CRDT_E_INVALID  # shift > 31
    assert call(cx=None) == call(r=None) == call(o=None) == CRDT_E_INVALID
    assert call(s=cs, i=None) == CRDT_E_INVALID  # the scatter mapping needs idx
    assert call(s=cs, i=didx.data_ptr(), n_out=n - 1) == call(s=cs, i=didx.data_ptr(), n_out=0) == CRDT_E_INVALID
    assert call(s=other.to(dev).c(), i=didx.data_ptr()) == CRDT_E_INVALID  # R differs between rep and sub
    assert call(r=abi.CReplica(None, None, None, 0)) == CRDT_E_INVALID
    assert call(o=abi.CReplicaOut(co.state, None, None)) == CRDT_E_INVALID  # out->tombs NULL although rep has tombs
    t = dr.tombs
    assert call(r=Replica(dr.state, TombBatch(None, t.keys, t.actors, t.counters), 0).c()) == CRDT_E_INVALID
    keep, out.state.keys = out.state.keys, dr.state.keys
    assert call(o=out.c()) == CRDT_E_INVALID  # an output array starting where an input array starts
    out.state.keys = keep
    eng.sync()
    for t in out.poisoned:
        assert bool((t == -1).all())
    # shift 31 and align 64 are the last values taken
    assert call(er=abi.CHeadroom(0, 1, 31, 64), tr=None) == 0
    eng.sync()


def test_empty_calls(eng, torch):
    """n_docs == 0 or n_out == 0: offsets[0] = 0 for entries and tombstones, nothing else."""
    dev = dev_of(torch)
    rep = cases()["sel-R3-layout0"].rep
    z32, z64 = np.zeros(0, U32), np.zeros(0, U64)
    empty = Replica(AWSetBatch(3, np.zeros(1, U32), z64, z32, z64, z64), TombBatch(np.zeros(1, U32), z64, z32, z64), 1)
    room = Headroom(2, 1, 0, 8)
    for r, n_out in ((rep, 0), (empty, 0), (empty, 4)):
        out = poisoned(torch, max(n_out, 1), 3, 8, 8)
        eng.replica_repack_async(r.to(dev), out, n_out=n_out, entry_room=room, tomb_room=room)
        eng.sync()
        for o in (out.state.offsets, out.tombs.offsets):
            h = _np(o, U32)
            assert h[0] == 0 and (h[1:] == ONES32).all()
        for t in out.poisoned:
            if t is not out.state.offsets and t is not out.tombs.offsets:
                assert bool((t == -1).all())
    out = poisoned(torch, 1, 3, 8, 8)
    eng.replica_repack_async(empty.to(dev), out, sub=rep.to(dev), idx=words(torch, np.arange(rep.n_docs, dtype=U32)),
                             n_out=0, entry_room=room)
    eng.sync()
    assert _np(out.state.offsets, U32)[0] == 0 and _np(out.tombs.offsets, U32)[0] == 0
    assert bool((out.state.counts == -1).all()) and bool((out.state.keys == -1).all())


# ------------------------------------------------ 5. determinism, capture, streams

def test_run_to_run_identity(eng, torch):
    """No atomic decides a position: two runs give the same bits."""
    for name in ("gather-doubling", "sct-edge-slack1"):
        c, ref = cases()[name], case_ref(name)
        a, b = launch(eng, torch, c, ref), launch(eng, torch, c, ref)
        eng.sync()
        for x, y in zip(tensors(a), tensors(b)):
            assert torch.equal(x, y)


def test_graph_capture(torch):
    """Both mappings captured on a reserved context and replayed with idx and *n_idx
    changed in between equal the reference; on an unreserved context the capture is
    refused with CRDT_E_WORKSPACE and launches nothing."""
    dev = dev_of(torch)
    c = cases()["sct-scan-1025"]
    rep, sub = c.rep, c.sub
    n, m, R = rep.n_docs, sub.n_docs, 2
    rng = np.random.default_rng(78)
    runs = [(rng.choice(n, m, replace=False).astype(U32), k) for k in (m, 100, 0)]
    er, tr = (2, 1, 0, 2), (1, 0, 0, 1)
    hr, ht = room_of(er), room_of(tr)
    te = 2 * (int(rep.state.offsets[-1]) + int(sub.state.offsets[-1])) + 4 * n
    tt = int(rep.tombs.offsets[-1]) + int(sub.tombs.offsets[-1]) + n
    e = crdtgpu.Engine(0)
    try:
        dr, ds = rep.to(dev), sub.to(dev)
        idxd = torch.zeros(m, dtype=torch.int32, device=dev)
        nd = torch.zeros(1, dtype=torch.int32, device=dev)
        o_sct = poisoned(torch, n, R, te, tt)
        o_sel = poisoned(torch, m, R, te, tt)
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.replica_repack_async(dr, o_sct, ds, idxd, nd, n, hr, ht, stream=torch.cuda.current_stream())
        assert ei.value.code == CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        for t in o_sct.poisoned:
            assert bool((t == -1).all())
        e.reserve(n)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.replica_repack_async(dr, o_sel, None, idxd, nd, m, hr, ht, stream=torch.cuda.current_stream())
            e.replica_repack_async(dr, o_sct, ds, idxd, nd, n, hr, ht, stream=torch.cuda.current_stream())
        for idx, k in runs + runs[:1]:
            idxd.copy_(words(torch, idx))
            nd.fill_(k)
            repoison(o_sct)
            repoison(o_sel)
            g.replay()
            e.sync(torch.cuda.current_stream())
            assert_repack(o_sel, replica_repack_ref(rep, None, idx, k, m, er, tr, te, tt))
            assert_repack(o_sct, replica_repack_ref(rep, sub, idx, k, n, er, tr, te, tt))
    finally:
        e.close()


def test_ordering_across_two_streams(eng, torch):
    """Calls on two streams share the context's workspace: each is ordered after the one before."""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    got = []
    for name, s in (("gather-doubling", s1), ("sct-scan-1025", s2), ("sel-R64-layout3", s1), ("sct-edge-slack0", s2)):
        c, ref = cases()[name], case_ref(name)
        with torch.cuda.stream(s):
            got.append((launch(eng, torch, c, ref, stream=s), ref))
    eng.sync(s1)
    eng.sync(s2)
    for out, ref in got:
        assert_repack(out, ref)


# ---------------------------------------------------------------- 6. rounds

def n_spill(sp):
    return int(_np(sp.n_spill, U32)[0])  # the 4 bytes a caller reads back


def compacted(eng, torch, target, n, R):
    out = poisoned(torch, n, R, target.state.keys.numel(), target.tombs.keys.numel())
    eng.replica_select_async(target.as_replica() if hasattr(target, "as_replica") else target, out)
    return out


def test_delta_round_spills_when_packed_and_fits_after_the_repack(eng, torch):
    """(a) the sparse delta round on PACKED replicas spills; (b) after the repack with the
    rounds' policy the same round places every document, the repack's output taken as the
    in-place target with no copy; (d) compacted, the result is the full exchange.  Nothing
    is downloaded in between but n_spill."""
    dev = dev_of(torch)
    m = delta_round_model()
    work, packed = m["work"], m["packed"]
    n, R, k = packed[0].n_docs, packed[0].state.R, 256
    assert len(work) <= k
    room = room_of(ROUND_ROOM)

    def sparse_round(ra, rb):
        """digest x 2, digest_diff, select x 2, delta exchange, in-place scatter x 2 -> the spill buffers."""
        dig = [torch.empty(2 * n, dtype=torch.int64, device=dev) for _ in range(2)]
        for r, d in zip((ra, rb), dig):
            eng.digest_async(r.state, d, r.tombs)
        cmp = CompareBuffers(n, device=dev)
        eng.digest_diff_async(dig[0], dig[1], n, cmp)
        sa, sb = (ReplicaBuffers(k, R, 40 * k, 40 * k, device=dev) for _ in range(2))
        eng.replica_select_async(ra, sa, cmp.worklist, cmp.n_work, k)
        eng.replica_select_async(rb, sb, cmp.worklist, cmp.n_work, k)
        yab, yba = (OutBuffers(k, R, 80 * k, device=dev) for _ in range(2))
        eng.delta_exchange_async(sa.as_replica(), sb.as_replica(), yab, yba)
        sps = []
        for r, y, s in ((ra, yab, sa), (rb, yba, sb)):
            sp = spill_buffers(torch, k)
            eng.replica_scatter_inplace_async(r, Replica(y.as_batch(), s.tombs, 0, s.doc_actor), cmp.worklist, sp,
                                              cmp.n_work)
            sps.append(sp)
        eng.sync()
        return [n_spill(sp) for sp in sps]

    # (a)
    got = sparse_round(*(r.to(dev) for r in packed))
    assert got == [len(r.spill_j) for r in m["on_packed"]] and sum(got) >= 1
    # (b) repack, then the round onto the repack's own buffers
    outs = []
    for r in packed:
        es, ts = repack_slots(r.state.counts, r.tombs.counts, room, room)
        out = poisoned(torch, n, R, es + SPARE, ts + SPARE)
        out.entry_slots, out.tomb_slots = es, ts
        eng.replica_repack_async(r.to(dev), out, entry_room=room, tomb_room=room)
        outs.append(out)
    assert all(isinstance(InplaceTarget.of(o), InplaceTarget) for o in outs)
    ra, rb = (o.as_replica() for o in outs)
    assert ra.state.keys.data_ptr() == outs[0].state.keys.data_ptr()  # no copy
    assert sparse_round(ra, rb) == [0, 0]
    for o, r in zip(outs, m["roomy"]):  # the layout the model repacked to
        assert (_np(o.state.offsets, U32)[: n + 1] == r.state.offsets).all()
        assert (_np(o.tombs.offsets, U32)[: n + 1] == r.tombs.offsets).all()
    # (d)
    for o, w in zip(outs, m["want"]):
        c = compacted(eng, torch, o, n, R)
        eng.sync()
        c.entry_slots, c.tomb_slots = c.state.keys.numel(), c.tombs.keys.numel()
        assert_replica(c, as_ref(w))


def test_apply_round_spill_then_repack_fallback_then_everything_fits(eng, torch):
    """(a) select, apply, in-place scatter on the PACKED replica: documents spill; (c) the
    fallback through the repack's scatter mapping with the rounds' policy, then the same ops
    on the same documents again: everything is placed; (d) both rounds equal the oracle's
    apply of the whole batch, compacted."""
    dev = dev_of(torch)
    m = apply_round_model()
    rep, idx, part = m["packed"], m["idx"], m["part"]
    n, R, k = rep.n_docs, rep.state.R, len(idx)
    room = room_of(ROUND_ROOM)
    didx = words(torch, idx)
    pops = int(part.op_off[-1])

    def sparse_apply(target_rep, e_sel, t_sel):
        sel = ReplicaBuffers(k, R, e_sel, t_sel, device=dev)
        eng.replica_select_async(target_rep, sel, didx, None, k)
        so, st = OutBuffers(k, R, e_sel + pops, device=dev), TombBuffers(k, t_sel + pops, device=dev)
        dpart = part.to(dev)
        dpart.doc_actor = sel.doc_actor
        eng.apply_async(sel.state.as_batch(), dpart, so, sel.tombs, st)
        sub = Replica(so.as_batch(), st, 0, sel.doc_actor)
        sp = spill_buffers(torch, k)
        eng.replica_scatter_inplace_async(target_rep, sub, didx, sp)
        return sub, sp, (e_sel + pops, t_sel + pops)

    dr = rep.to(dev)
    sub, sp, (e_sub, t_sub) = sparse_apply(dr, int(rep.state.offsets[-1]), int(rep.tombs.offsets[-1]))
    # the fallback: the spilled documents selected, then scattered back WITH headroom
    spilled = ReplicaBuffers(k, R, e_sub, t_sub, device=dev)
    eng.replica_select_async(sub, spilled, sp.spill_j, sp.n_spill, k)
    back = m["back"]
    out = poisoned(torch, n, R, back.total["e"] + SPARE, back.total["t"] + SPARE)
    out.entry_slots, out.tomb_slots = back.total["e"], back.total["t"]
    eng.replica_repack_async(dr, out, spilled.as_replica(), sp.spill_doc, sp.n_spill, n, room, room)
    eng.sync()
    assert n_spill(sp) == len(m["ref1"].spill_j) >= 1  # (a)
    assert_repack(out, back)
    # round 2 onto the repack's own buffers
    sub2, sp2, _ = sparse_apply(out.as_replica(), out.entry_slots, out.tomb_slots)
    eng.sync()
    assert n_spill(sp2) == 0  # (c)
    c = compacted(eng, torch, out, n, R)
    eng.sync()
    c.entry_slots, c.tomb_slots = c.state.keys.numel(), c.tombs.keys.numel()
    assert_replica(c, as_ref(m["want2"]))  # (d)
