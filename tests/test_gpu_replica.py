"""GPU: crdt_replica_select_async / crdt_replica_scatter_async (csrc/replica.hip)
against replica_select_ref / replica_scatter_ref (tests/test_replica_model.py),
bit-exact.

Every output buffer is pre-filled with poison (words all-ones), so each word read
back was written by the call, and entry and tombstone slots at or past the
totals must still hold it.  The kernels work in these units, and the cases
(test_replica_model.select_cases / scatter_cases / edge_docs) are sized around them:
  kRepScanChunk   = 1,024 output documents per workgroup of the offset scan,
  kRepPartStep    = 1,024 partial sums per step of the one-workgroup partials scan
                    (2^20 + 1 documents: it steps),
  kRepGatherChunk = 2,048 output positions per gather step,
  kRepRun         = 1,024 documents of a gather chunk staged in LDS at most.
"""

import ctypes

import numpy as np
import pytest

import crdtgpu
from crdtgpu import CRDT_E_CAPACITY, CRDT_E_INVALID, CRDT_E_WORKSPACE, abi
from crdtgpu.batch import (AWSetBatch, CompareBuffers, OutBuffers, Replica, ReplicaBuffers, TombBatch, TombBuffers,
                           _np)
from test_gpu_compare import _code, dev_of
from test_replica_model import (K_PART, K_SCAN, U32, U64, apply_round_case, big_replica,
                                big_scatter_case, delta_round_case, replica_scatter_ref, replica_select_ref,
                                scatter_cases, select_cases)

pytestmark = pytest.mark.gpu

ONES32 = 2 ** 32 - 1
MAXK = 2 ** 64 - 1
COLS = ("keys", "actors", "counters")


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

def poisoned(torch, n_out, R, e_slots, t_slots, tombs="all", actors=True):
    """Device output buffers filled with all-ones words.  tombs: "all", "off" (only
    the tombstone offsets and counts are passed) or "none" (out->tombs == NULL)."""
    out = ReplicaBuffers(n_out, R, e_slots, t_slots, device=dev_of(torch), tombs=tombs != "none", actors=actors)
    ts = [out.state.offsets, out.state.counts, out.state.keys, out.state.actors, out.state.counters, out.state.vv]
    if out.tombs is not None:
        ts += [out.tombs.offsets, out.tombs.counts, out.tombs.keys, out.tombs.actors, out.tombs.counters]
    if out.doc_actor is not None:
        ts.append(out.doc_actor)
    for t in ts:
        t.fill_(-1)
    out.poisoned = ts
    if tombs == "off":
        out.tombs.keys = out.tombs.actors = out.tombs.counters = None
    return out


def repoison(out):
    for t in out.poisoned:
        t.fill_(-1)


def assert_replica(out, ref):
    """A poisoned device output equals ref (ReplicaRef): every word of the offsets,
    counts, clocks and actors, the entries and tombstones below the totals written,
    every slot at or past them still poison."""
    w, n, R = ref.rep, out.n_docs, out.R
    st = out.state
    assert (_np(st.offsets, U32)[: n + 1] == w.state.offsets).all(), "offsets"
    assert (_np(st.counts, U32)[:n] == w.state.counts).all(), "counts"
    assert (_np(st.vv, U64)[: n * R] == w.state.vv).all(), "vv"
    if out.doc_actor is not None:
        assert (_np(out.doc_actor, U32)[:n] == w.doc_actor).all(), "doc_actor"
    sets = [("entry ", st, w.state, ref.n_e, out.entry_slots)]
    if out.tombs is not None:
        assert (_np(out.tombs.offsets, U32)[: n + 1] == w.tombs.offsets).all(), "tomb offsets"
        assert (_np(out.tombs.counts, U32)[:n] == w.tombs.counts).all(), "tomb counts"
        if out.tombs.keys is not None:
            sets.append(("tomb ", out.tombs, w.tombs, ref.n_t, out.tomb_slots))
    else:
        assert int(w.tombs.offsets[-1]) == 0
    for what, got, want, m, slots in sets:
        for f in COLS:
            g = _np(getattr(got, f), U32 if f == "actors" else U64)
            x = getattr(want, f)[:m]
            if not (g[:m] == x).all():
                i = int(np.nonzero(g[:m] != x)[0][0])
                raise AssertionError("%s%s differs first at %d of %d: gpu %d, expected %d" % (what, f, i, m, g[i], x[i]))
            assert m <= slots and (g[m:] == (ONES32 if f == "actors" else MAXK)).all(), \
                what + f + " written at or past the total"


def words(torch, a):
    if a is None:
        return None
    a = np.ascontiguousarray(a, U32)
    t = torch.from_numpy(a.view(np.int32).copy()).to(dev_of(torch))
    return t if t.numel() else torch.zeros(1, dtype=torch.int32, device=dev_of(torch))


def word(torch, v):
    return None if v is None else torch.tensor([v], dtype=torch.int64, device=dev_of(torch)).to(torch.int32)


def select_on_device(eng, torch, rep, idx=None, n_idx=None, n_out=None, spare=3, entry_slots=None, tomb_slots=None,
                     tombs=None, actors=True, dev_rep=None, ref=None, stream=None):
    """(poisoned output after one call, ref); the call is not synced."""
    ref = ref or replica_select_ref(rep, idx, n_idx, n_out, entry_slots, tomb_slots)
    n_out = rep.n_docs if n_out is None else n_out
    te, tt = int(ref.rep.state.offsets[-1]), int(ref.rep.tombs.offsets[-1])
    es = te + spare if entry_slots is None else entry_slots
    ts = tt + spare if tomb_slots is None else tomb_slots
    out = poisoned(torch, n_out, rep.state.R, max(es, te) + spare, max(ts, tt) + spare,
                   tombs or ("all" if rep.tombs is not None else "none"), actors)
    out.entry_slots, out.tomb_slots = es, ts  # the limits the call is given: slots past them stay poison too
    eng.replica_select_async(dev_rep or rep.to(dev_of(torch)), out, words(torch, idx), word(torch, n_idx), n_out,
                             stream=stream)
    return out, ref


def scatter_on_device(eng, torch, rep, sub, idx, n_idx=None, spare=3, entry_slots=None, tomb_slots=None, tombs=None,
                      actors=True, dev_rep=None, dev_sub=None, ref=None):
    ref = ref or replica_scatter_ref(rep, sub, idx, n_idx, entry_slots, tomb_slots)
    te, tt = int(ref.rep.state.offsets[-1]), int(ref.rep.tombs.offsets[-1])
    es = te + spare if entry_slots is None else entry_slots
    ts = tt + spare if tomb_slots is None else tomb_slots
    any_t = rep.tombs is not None or sub.tombs is not None
    out = poisoned(torch, rep.n_docs, rep.state.R, max(es, te) + spare, max(ts, tt) + spare,
                   tombs or ("all" if any_t else "none"), actors)
    out.entry_slots, out.tomb_slots = es, ts
    dev = dev_of(torch)
    eng.replica_scatter_async(dev_rep or rep.to(dev), dev_sub or sub.to(dev), words(torch, idx), out,
                              word(torch, n_idx))
    return out, ref


def shifted(torch, t):
    """The same values in a tensor whose first element sits one element past an aligned address."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    big[1:].copy_(t)
    return big[1:]


# ------------------------------------------------- 1. the cases of the model file

@pytest.mark.parametrize("name", sorted(select_cases()))
def test_select_cases(eng, torch, name):
    """R 1 / 3 / 64; counts NULL and given, slack, stale non-zero slack; tombs NULL;
    doc_actor given and uniform; idx in any order and repeating; *n_idx below n_out,
    equal to it and 0; compaction at 1 / 1,023 / 1,024 / 1,025 documents; the gather
    edges (documents ending at 2,047 / 2,048 / 2,049, one over three chunks, more
    than 1,024 documents in one chunk, odd and even source offsets)."""
    rep, idx, n_idx, n_out = select_cases()[name]
    out, ref = select_on_device(eng, torch, rep, idx, n_idx, n_out)
    eng.sync()
    assert_replica(out, ref)


@pytest.mark.parametrize("name", sorted(scatter_cases()))
def test_scatter_cases(eng, torch, name):
    """tombs NULL on rep, on sub and on both; replacements longer, shorter and empty,
    in entries and tombstones independently; idx descending; *n_idx 0, partial and
    NULL; the scan and gather edges."""
    rep, sub, idx, n_idx = scatter_cases()[name]
    out, ref = scatter_on_device(eng, torch, rep, sub, idx, n_idx)
    eng.sync()
    assert_replica(out, ref)


def test_output_forms(eng, torch):
    """out->doc_actor == NULL; out->tombs with offsets and counts alone, and NULL, when
    no input has tombstones: what is passed is zeroed."""
    rep, idx, n_idx, n_out = select_cases()["R3-layout0"]
    out, ref = select_on_device(eng, torch, rep, idx, n_idx, n_out, actors=False)
    eng.sync()
    assert_replica(out, ref)
    bare, bidx, bn, bo = select_cases()["R3-layout1"]
    assert bare.tombs is None
    for form in ("off", "none", "all"):
        out, ref = select_on_device(eng, torch, bare, bidx, bn, bo, tombs=form)
        eng.sync()
        assert_replica(out, ref)
    rep2, sub2, idx2, n2 = scatter_cases()["R3-tombs-none"]
    for form in ("off", "none"):
        out, ref = scatter_on_device(eng, torch, rep2, sub2, idx2, n2, tombs=form, actors=form == "off")
        eng.sync()
        assert_replica(out, ref)


# ----------------------------------------------------- 2. 2^20 + 1 documents

def test_partials_scan_steps(eng, torch):
    """1,048,577 documents (one past 1,024 chunks of 1,024) of 0 or 1 entries and 0
    or 1 tombstones: compaction, and a scatter replacing 5,000 of them."""
    rep, sub, idx = big_scatter_case()
    assert (rep.n_docs + K_SCAN - 1) // K_SCAN == K_PART + 1
    dev_rep = rep.to(dev_of(torch))
    out, ref = select_on_device(eng, torch, rep, dev_rep=dev_rep)
    eng.sync()
    assert_replica(out, ref)
    del out
    out, ref = scatter_on_device(eng, torch, rep, sub, idx, dev_rep=dev_rep)
    eng.sync()
    assert_replica(out, ref)


# ------------------------------------------------------ 3. pair alignment

@pytest.mark.parametrize("where", ["inputs", "output", "both"])
def test_unaligned_columns_give_the_same_result(eng, torch, where):
    """Column pointers one element off 16 B: the gather goes element by element on
    that side, and the result is identical."""
    rep, sub, idx, n_idx = scatter_cases()["edge-slack1"]
    dev = dev_of(torch)
    dr, ds = rep.to(dev), sub.to(dev)
    if where != "output":
        for cols in (dr.state, ds.tombs):
            for f in COLS:
                setattr(cols, f, shifted(torch, getattr(cols, f)))
                assert getattr(cols, f).data_ptr() % (8 if f == "actors" else 16) != 0
    ref = replica_scatter_ref(rep, sub, idx, n_idx)
    te, tt = int(ref.rep.state.offsets[-1]), int(ref.rep.tombs.offsets[-1])
    out = poisoned(torch, rep.n_docs, 2, te + 3, tt + 3)
    if where != "inputs":
        for cols in (out.state, out.tombs):
            for f in COLS:
                setattr(cols, f, shifted(torch, getattr(cols, f))[: getattr(cols, f).numel() - 1])
        out.entry_slots, out.tomb_slots = te + 2, tt + 2
    eng.replica_scatter_async(dr, ds, words(torch, idx), out)
    eng.sync()
    assert_replica(out, ref)


# ---------------------------------------- 4. outputs of other calls as they stand

def test_apply_and_delta_exchange_outputs_as_they_stand(eng, torch):
    """A device apply output (tombstones at tombs.offsets[d] + op_off[d], slack never
    written) compacted, and a delta-exchange output (join layout) selected, with no
    copy in between."""
    dev = dev_of(torch)
    rep, idx, part, full = apply_round_case()
    n, R = rep.n_docs, rep.state.R
    nops = int(full.op_off[-1])
    ao = OutBuffers(n, R, int(rep.state.offsets[-1]) + nops, device=dev)
    at = TombBuffers(n, int(rep.tombs.offsets[-1]) + nops, device=dev)
    for t in (ao.keys, ao.actors, ao.counters, at.keys, at.actors, at.counters):
        t.fill_(-1)  # what apply does not write is never read
    dr = rep.to(dev)
    eng.apply_async(dr.state, full.to(dev), ao, dr.tombs, at)
    eng.sync()
    host = Replica(AWSetBatch(R, *(_np(getattr(ao, f), U32 if f in ("offsets", "actors") else U64)
                                   for f in ("offsets", "keys", "actors", "counters", "vv")), counts=_np(ao.counts, U32)),
                   TombBatch(_np(at.offsets, U32), _np(at.keys, U64), _np(at.actors, U32), _np(at.counters, U64),
                             counts=_np(at.counts, U32)), 0, rep.doc_actor)
    assert (np.diff(host.tombs.offsets.astype(np.int64)) > host.tombs.counts).any()
    out, ref = select_on_device(eng, torch, host, dev_rep=Replica(ao.as_batch(), at, 0, dr.doc_actor))
    eng.sync()
    assert_replica(out, ref)
    a, b, work, _, _ = delta_round_case()
    da, db = a.to(dev), b.to(dev)
    slots = int(a.state.offsets[-1]) + int(b.state.offsets[-1])
    xab, xba = (OutBuffers(a.n_docs, R, slots, device=dev) for _ in range(2))
    for o in (xab, xba):
        for t in (o.keys, o.actors, o.counters):
            t.fill_(-1)
    eng.delta_exchange_async(da, db, xab, xba)
    eng.sync()
    hx = Replica(AWSetBatch(R, *(_np(getattr(xab, f), U32 if f in ("offsets", "actors") else U64)
                                 for f in ("offsets", "keys", "actors", "counters", "vv")), counts=_np(xab.counts, U32)),
                 a.tombs, a.actor, a.doc_actor)
    sel = np.arange(0, a.n_docs, 7).astype(U32)
    out, ref = select_on_device(eng, torch, hx, sel, None, len(sel),
                                dev_rep=Replica(xab.as_batch(), da.tombs, a.actor, da.doc_actor))
    eng.sync()
    assert_replica(out, ref)


# ------------------------------------------------- 5. agreement with select / scatter

def test_state_part_is_what_select_and_scatter_write(eng, torch):
    """out->state equals the output of crdt_awset_select_async / crdt_awset_scatter_async
    run on the same arguments, bit for bit, offsets included."""
    dev = dev_of(torch)

    def same(o1, o2, n, R, total):
        for f, m in (("offsets", n + 1), ("counts", n), ("vv", n * R), ("keys", total), ("actors", total),
                     ("counters", total)):
            assert torch.equal(getattr(o1, f)[:m], getattr(o2, f)[:m]), f

    for name in ("R3-layout3", "R64-layout2", "edge-compact-slack1", "edge-permuted", "compact-1025"):
        rep, idx, n_idx, n_out = select_cases()[name]
        out, ref = select_on_device(eng, torch, rep, idx, n_idx, n_out)
        plain = OutBuffers(n_out, rep.state.R, out.entry_slots, device=dev)
        eng.select_async(rep.state.to(dev), plain, words(torch, idx), word(torch, n_idx), n_out, out.entry_slots)
        eng.sync()
        same(out.state, plain, n_out, rep.state.R, ref.n_e)
    for name in ("R3-tombs-both", "R64-descending", "R1-n_idx-17", "edge-slack0", "scan-1025"):
        rep, sub, idx, n_idx = scatter_cases()[name]
        out, ref = scatter_on_device(eng, torch, rep, sub, idx, n_idx)
        plain = OutBuffers(rep.n_docs, rep.state.R, out.entry_slots, device=dev)
        eng.scatter_async(rep.state.to(dev), sub.state.to(dev), words(torch, idx), plain, word(torch, n_idx),
                          out.entry_slots)
        eng.sync()
        same(out.state, plain, rep.n_docs, rep.state.R, ref.n_e)


# ---------------------------------------------------------------- 6. errors

def test_reported_conditions(eng, torch):
    """Every condition crdt_ctx_sync reports: the clamps and what is still written."""
    rep, idx, _, n_out = select_cases()["R3-layout2"]
    # *n_idx above n_out: clamped
    out, ref = select_on_device(eng, torch, rep, idx, n_out + 5, n_out)
    assert ref.capacity and not ref.invalid and _code(eng.sync) == CRDT_E_CAPACITY
    assert_replica(out, ref)
    # an idx[j] that is no document: empty, actor 0
    bad = idx.copy()
    bad[[3, 77]] = [300, ONES32]
    out, ref = select_on_device(eng, torch, rep, bad, None, n_out)
    assert ref.invalid and not ref.capacity and _code(eng.sync) == CRDT_E_INVALID
    assert_replica(out, ref)
    # live counts above their slots, entries and tombstones, on either source: clamped
    srep, ssub, sidx, _ = scatter_cases()["R3-tombs-both"]

    def bumped(r, which, d):
        cols = getattr(r, which)
        counts = cols.counts.copy()
        counts[d] += 9
        if which == "state":
            return Replica(AWSetBatch(r.state.R, cols.offsets, cols.keys, cols.actors, cols.counters, cols.vv,
                                      counts=counts), r.tombs, r.actor, r.doc_actor)
        return Replica(r.state, TombBatch(cols.offsets, cols.keys, cols.actors, cols.counters, counts=counts), r.actor,
                       r.doc_actor)

    kept = int(np.setdiff1d(np.arange(rep.n_docs), sidx)[0])  # a document the scatter does not replace
    for which in ("state", "tombs"):
        out, ref = select_on_device(eng, torch, bumped(rep, which, int(idx[0])), idx, None, n_out)
        assert ref.capacity and _code(eng.sync) == CRDT_E_CAPACITY
        assert_replica(out, ref)
        for r2, s2 in ((bumped(rep, which, kept), ssub), (rep, bumped(ssub, which, 4))):
            out, ref = scatter_on_device(eng, torch, r2, s2, sidx)
            assert ref.capacity and _code(eng.sync) == CRDT_E_CAPACITY
            assert_replica(out, ref)
    # a total one above its slots, entries and tombstones independently: offsets and totals
    # exact, nothing written at or past the slots of the exceeded array, the other complete
    full = replica_select_ref(rep, idx, None, n_out)
    te, tt = full.n_e, full.n_t
    for es, ts in ((te - 1, tt), (te, tt - 1), (te - 1, tt - 1), (0, 0)):
        out, ref = select_on_device(eng, torch, rep, idx, None, n_out, entry_slots=es, tomb_slots=ts)
        assert ref.capacity and (ref.n_e, ref.n_t) == (es, ts) and _code(eng.sync) == CRDT_E_CAPACITY
        assert_replica(out, ref)
    srep = rep
    full = replica_scatter_ref(srep, ssub, sidx)
    te, tt = full.n_e, full.n_t
    for es, ts in ((te - 1, tt), (te, tt - 1)):
        out, ref = scatter_on_device(eng, torch, srep, ssub, sidx, entry_slots=es, tomb_slots=ts)
        assert ref.capacity and _code(eng.sync) == CRDT_E_CAPACITY
        assert_replica(out, ref)
    # scatter: *n_idx above sub's documents; an idx[j] that is no document; a document named twice
    out, ref = scatter_on_device(eng, torch, srep, ssub, sidx, ssub.n_docs + 1)
    assert ref.capacity and _code(eng.sync) == CRDT_E_CAPACITY
    assert_replica(out, ref)
    for j, v in ((5, 300), (9, int(sidx[2]))):
        bad = sidx.copy()
        bad[j] = v
        out, ref = scatter_on_device(eng, torch, srep, ssub, bad)
        assert ref.invalid and _code(eng.sync) == CRDT_E_INVALID
        assert_replica(out, ref)
    eng.sync()


def test_invalid_arguments(eng, torch):
    """What the call itself returns CRDT_E_INVALID for; nothing is launched."""
    dev = dev_of(torch)
    rep, sub, idx, _ = scatter_cases()["R3-tombs-both"]
    other = scatter_cases()["R1-tombs-both"][1]
    dr, ds, didx = rep.to(dev), sub.to(dev), words(torch, idx)
    out = poisoned(torch, rep.n_docs, 3, 4000, 2000)
    lib, ctx = abi.lib(), eng._ctx
    cr, cs, co = dr.c(), ds.c(), out.c()

    def sel(r=cr, o=co, c=ctx):
        return lib.crdt_replica_select_async(c, ctypes.byref(r) if r is not None else None, None, None, rep.n_docs,
                                             4000, 2000, ctypes.byref(o) if o is not None else None, None)

    def sct(r=cr, s=cs, i=didx.data_ptr(), o=co):
        return lib.crdt_replica_scatter_async(ctx, ctypes.byref(r) if r is not None else None,
                                              ctypes.byref(s) if s is not None else None, i, None, 4000, 2000,
                                              ctypes.byref(o) if o is not None else None, None)

    assert sel(c=None) == sel(r=None) == sel(o=None) == CRDT_E_INVALID
    assert sct(r=None) == sct(s=None) == sct(i=None) == sct(o=None) == CRDT_E_INVALID
    assert sel(r=abi.CReplica(None, None, None, 0)) == CRDT_E_INVALID  # no state
    assert sel(o=abi.CReplicaOut(None, co.tombs, None)) == CRDT_E_INVALID  # out->state NULL
    assert sel(o=abi.CReplicaOut(co.state, None, None)) == CRDT_E_INVALID  # out->tombs NULL although rep has tombs
    no_keys = poisoned(torch, rep.n_docs, 3, 4000, 2000, tombs="off")
    assert sel(o=no_keys.c()) == CRDT_E_INVALID  # ... or without its columns
    assert sct(s=other.to(dev).c()) == CRDT_E_INVALID  # R differs between rep and sub
    t = dr.tombs
    assert sel(r=Replica(dr.state, TombBatch(None, t.keys, t.actors, t.counters), 0).c()) == CRDT_E_INVALID  # no offsets
    assert sct(s=Replica(ds.state, TombBatch(None, t.keys, t.actors, t.counters), 0).c()) == CRDT_E_INVALID
    # an output array starting where an input array of the same kind starts
    for holder, f in ((out.state, "offsets"), (out.state, "keys"), (out.state, "vv"), (out.tombs, "offsets"),
                      (out.tombs, "counters")):
        keep = getattr(holder, f)
        src = dr.tombs if holder is out.tombs else dr.state
        setattr(holder, f, getattr(src, f))
        assert sel(o=out.c()) == CRDT_E_INVALID, f
        setattr(holder, f, getattr(ds.tombs if holder is out.tombs else ds.state, f))
        assert sct(o=out.c()) == CRDT_E_INVALID, f
        setattr(holder, f, keep)
    keep, out.doc_actor = out.doc_actor, ds.doc_actor
    assert ds.doc_actor is not None and sct(o=out.c()) == CRDT_E_INVALID
    out.doc_actor = keep
    eng.sync()
    for t in out.poisoned:
        assert bool((t == -1).all())


def test_empty_calls(eng, torch):
    """n_docs == 0 or n_out == 0: offsets[0] = 0 for entries and tombstones, nothing else."""
    dev = dev_of(torch)
    rep = select_cases()["R3-layout0"][0]
    z32, z64 = np.zeros(0, U32), np.zeros(0, U64)
    empty = Replica(AWSetBatch(3, np.zeros(1, U32), z64, z32, z64, z64), TombBatch(np.zeros(1, U32), z64, z32, z64), 1)
    for r, n_out in ((rep, 0), (empty, 0), (empty, 4)):
        out = poisoned(torch, max(n_out, 1), 3, 8, 8)
        eng.replica_select_async(r.to(dev), out, None, None, n_out)
        eng.sync()
        for o in (out.state.offsets, out.tombs.offsets):
            h = _np(o, U32)
            assert h[0] == 0 and (h[1:] == ONES32).all()
        for t in out.poisoned:
            if t is not out.state.offsets and t is not out.tombs.offsets:
                assert bool((t == -1).all())
    out = poisoned(torch, 1, 3, 8, 8)
    eng.replica_scatter_async(empty.to(dev), rep.to(dev), words(torch, np.arange(rep.n_docs, dtype=U32)), out)
    eng.sync()
    assert _np(out.state.offsets, U32)[0] == 0 and _np(out.tombs.offsets, U32)[0] == 0
    assert bool((out.state.counts == -1).all()) and bool((out.state.keys == -1).all())


# --------------------------------------------------------------- 7. capture

def test_graph_capture(torch):
    """Select and scatter captured on a reserved context and replayed twice with idx
    and *n_idx changed in between equal the eager calls; on an unreserved context the
    capture is refused with CRDT_E_WORKSPACE and launches nothing (scatter: more than
    1,024 documents; select: more than 1,024 scan chunks)."""
    dev = dev_of(torch)
    rep, sub, _, _ = scatter_cases()["scan-1025"]
    n, m, R = rep.n_docs, sub.n_docs, 2
    rng = np.random.default_rng(77)
    runs = [(rng.choice(n, m, replace=False).astype(U32), k) for k in (m, 100, 0)]
    big = big_replica()
    e = crdtgpu.Engine(0)
    try:
        dr, ds, dbig = rep.to(dev), sub.to(dev), big.to(dev)
        idxd = torch.zeros(m, dtype=torch.int32, device=dev)
        nd = torch.zeros(1, dtype=torch.int32, device=dev)
        te = int(rep.state.offsets[-1]) + int(sub.state.offsets[-1])
        tt = int(rep.tombs.offsets[-1]) + int(sub.tombs.offsets[-1])
        o_sct = poisoned(torch, n, R, te, tt)
        o_sel = poisoned(torch, m, R, te, tt)
        o_big = poisoned(torch, big.n_docs, 1, big.n_docs, big.n_docs)  # never written: the call is refused
        for call in (lambda s: e.replica_scatter_async(dr, ds, idxd, o_sct, nd, stream=s),
                     lambda s: e.replica_select_async(dbig, o_big, None, None, big.n_docs, stream=s)):
            g0 = torch.cuda.CUDAGraph()
            with pytest.raises(crdtgpu.CrdtError) as ei:
                with torch.cuda.graph(g0):
                    call(torch.cuda.current_stream())
            assert ei.value.code == CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        for t in o_sct.poisoned + o_big.poisoned:
            assert bool((t == -1).all())
        e.reserve(n)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.replica_select_async(dr, o_sel, idxd, nd, m, stream=torch.cuda.current_stream())
            e.replica_scatter_async(dr, ds, idxd, o_sct, nd, stream=torch.cuda.current_stream())
        for idx, k in runs + runs[:1]:
            idxd.copy_(words(torch, idx))
            nd.fill_(k)
            repoison(o_sct)
            repoison(o_sel)
            g.replay()
            e.sync(torch.cuda.current_stream())
            assert_replica(o_sel, replica_select_ref(rep, idx, k, m, te, tt))
            assert_replica(o_sct, replica_scatter_ref(rep, sub, idx, k, te, tt))
    finally:
        e.close()


# ---------------------------------------------------------------- 8. rounds

def test_sparse_apply_round(eng, torch):
    """replica_select, apply, replica_scatter with nothing downloaded in between equals
    apply over the whole batch (empty op lists elsewhere), compacted."""
    dev = dev_of(torch)
    rep, idx, part, full = apply_round_case()
    n, R, m = rep.n_docs, rep.state.R, len(idx)
    dr, didx = rep.to(dev), words(torch, idx)
    # the whole batch, for the expectation
    nops = int(full.op_off[-1])
    fo = OutBuffers(n, R, int(rep.state.offsets[-1]) + nops, device=dev)
    ft = TombBuffers(n, int(rep.tombs.offsets[-1]) + nops, device=dev)
    eng.apply_async(dr.state, full.to(dev), fo, dr.tombs, ft)
    want = poisoned(torch, n, R, fo.slots, int(ft.keys.numel()))
    eng.replica_select_async(Replica(fo.as_batch(), ft, 0, dr.doc_actor), want)
    # the sparse round
    e_sel, t_sel = rep.state.live_slots(), int(rep.tombs.offsets[-1])
    sel = poisoned(torch, m, R, e_sel, t_sel)
    eng.replica_select_async(dr, sel, didx, None, m)
    pops = int(part.op_off[-1])
    so = OutBuffers(m, R, e_sel + pops, device=dev)
    st = TombBuffers(m, t_sel + pops, device=dev)
    dpart = part.to(dev)
    dpart.doc_actor = sel.doc_actor  # the selected actors, as they came out of the select
    eng.apply_async(sel.state.as_batch(), dpart, so, sel.tombs, st)
    got = poisoned(torch, n, R, want.entry_slots, want.tomb_slots)
    eng.replica_scatter_async(dr, Replica(so.as_batch(), st, 0, sel.doc_actor), didx, got)
    eng.sync()
    ne, nt = int(_np(want.state.offsets, U32)[n]), int(_np(want.tombs.offsets, U32)[n])
    assert ne > 0 and nt > 0
    for a, b in zip(got.poisoned, want.poisoned):
        assert torch.equal(a, b)
    ref = replica_select_ref(rep)
    assert not (_np(got.state.offsets, U32)[: n + 1] == ref.rep.state.offsets).all()  # the ops changed something


def test_sparse_delta_round(eng, torch):
    """digest (with tombs) of both replicas, digest_diff, the worklist, replica_select x 2,
    delta_exchange, replica_scatter x 2, nothing downloaded in between: the merged states
    go back with the selected tombstones and actors, and the result equals the full
    delta_exchange, compacted (3,000 documents, about 4 % differing)."""
    dev = dev_of(torch)
    a, b, work, _, _ = delta_round_case()
    n, R = a.n_docs, a.state.R
    da, db = a.to(dev), b.to(dev)
    slots = int(a.state.offsets[-1]) + int(b.state.offsets[-1])
    ta, tb = int(a.tombs.offsets[-1]), int(b.tombs.offsets[-1])
    # the full exchange, compacted, for the expectation
    xab, xba = (OutBuffers(n, R, slots, device=dev) for _ in range(2))
    eng.delta_exchange_async(da, db, xab, xba)
    want_a, want_b = poisoned(torch, n, R, slots, ta), poisoned(torch, n, R, slots, tb)
    eng.replica_select_async(Replica(xab.as_batch(), da.tombs, a.actor, da.doc_actor), want_a)
    eng.replica_select_async(Replica(xba.as_batch(), db.tombs, b.actor, db.doc_actor), want_b)
    # the sparse round
    dig_a = torch.empty(2 * n, dtype=torch.int64, device=dev)
    dig_b = torch.empty(2 * n, dtype=torch.int64, device=dev)
    eng.digest_async(da.state, dig_a, da.tombs)
    eng.digest_async(db.state, dig_b, db.tombs)
    cmp = CompareBuffers(n, device=dev)
    eng.digest_diff_async(dig_a, dig_b, n, cmp)
    m = 256  # an upper bound of the worklist the caller chose; *n_work is read on the device
    assert len(work) <= m
    sa, sb = poisoned(torch, m, R, 40 * m, 40 * m), poisoned(torch, m, R, 40 * m, 40 * m)
    eng.replica_select_async(da, sa, cmp.worklist, cmp.n_work, m)
    eng.replica_select_async(db, sb, cmp.worklist, cmp.n_work, m)
    ra, rb = sa.as_replica(), sb.as_replica()
    yab, yba = (OutBuffers(m, R, 80 * m, device=dev) for _ in range(2))
    eng.delta_exchange_async(ra, rb, yab, yba)
    got_a, got_b = poisoned(torch, n, R, slots, ta), poisoned(torch, n, R, slots, tb)
    eng.replica_scatter_async(da, Replica(yab.as_batch(), sa.tombs, 0, sa.doc_actor), cmp.worklist, got_a, cmp.n_work)
    eng.replica_scatter_async(db, Replica(yba.as_batch(), sb.tombs, 0, sb.doc_actor), cmp.worklist, got_b, cmp.n_work)
    eng.sync()
    assert (cmp.numpy()[2] == work).all()
    for got, want in ((got_a, want_a), (got_b, want_b)):
        for x, y in zip(got.poisoned, want.poisoned):
            assert torch.equal(x, y)
    assert not torch.equal(got_a.state.counts, da.state.counts)  # the exchange changed something
    assert (_np(got_b.doc_actor, U32) == 1).all() and (_np(got_a.doc_actor, U32) == 0).all()
