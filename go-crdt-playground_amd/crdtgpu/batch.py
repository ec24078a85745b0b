"""SoA batch containers matching include/crdtgpu.h.

A batch's arrays are either numpy arrays (host: the synchronous ``*_batch``
entry points) or torch tensors on a HIP device (the ``*_async`` entry points,
inputs resident in HBM).  Device tensors use torch.int32 / torch.int64, whose
bits are the ABI's u32 / u64.
"""

from __future__ import annotations

import ctypes

import numpy as np

import dataclasses

from .abi import (CAWSetBatch, CAWSetOut, CCompareOut, CDeltaOut, CDiffOut, CHeadroom, CMergeLog, COpBatch, CQueryBatch, CQueryOut, CReplica, CReplicaInplace, CReplicaOut, CSpillOut, CSrcBatch,
                  CTombBatch, CTombOut)

U32, U64 = np.uint32, np.uint64


def _is_torch(a) -> bool:
    return a is not None and type(a).__module__.startswith("torch")


def ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if not a.flags.c_contiguous:
            raise ValueError("array must be C-contiguous")
        return a.ctypes.data
    if not a.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return a.data_ptr()


def _np(a, dtype):
    if a is None:
        return None
    if _is_torch(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a).view(dtype) if a.dtype.itemsize == np.dtype(dtype).itemsize else \
        np.ascontiguousarray(a, dtype=dtype)


def _torch(a, device):
    import torch

    if a is None:
        return None
    if _is_torch(a):
        return a.to(device)
    sdt = {1: (np.uint8, torch.uint8), 4: (np.int32, torch.int32), 8: (np.int64, torch.int64)}[a.dtype.itemsize]
    return torch.from_numpy(np.ascontiguousarray(a).view(sdt[0])).to(device)


class AWSetBatch:
    """n_docs AWSet states: doc d owns slots [offsets[d], offsets[d+1]), live = counts[d]."""

    def __init__(self, R, offsets, keys, actors, counters, vv, counts=None):
        self.R = int(R)
        self.offsets, self.keys, self.actors, self.counters, self.vv, self.counts = (
            offsets, keys, actors, counters, vv, counts)

    @property
    def n_docs(self) -> int:
        return int(self.offsets.shape[0]) - 1

    def c(self) -> CAWSetBatch:
        return CAWSetBatch(self.n_docs, self.R, ptr(self.offsets), ptr(self.counts), ptr(self.keys),
                           ptr(self.actors), ptr(self.counters), ptr(self.vv))

    def numpy(self) -> "AWSetBatch":
        return AWSetBatch(self.R, _np(self.offsets, U32), _np(self.keys, U64), _np(self.actors, U32),
                          _np(self.counters, U64), _np(self.vv, U64), _np(self.counts, U32))

    def to(self, device) -> "AWSetBatch":
        return AWSetBatch(self.R, *(_torch(a, device) for a in (self.offsets, self.keys, self.actors,
                                                                  self.counters, self.vv)),
                          counts=_torch(self.counts, device))

    # -- host helpers ---------------------------------------------------
    @staticmethod
    def from_docs(R, docs, slack=0) -> "AWSetBatch":
        """docs: list of (entries [(key, actor, counter)] sorted by key, vv [R])."""
        n = len(docs)
        counts = np.array([len(e) for e, _ in docs], dtype=U32)
        caps = counts + U32(slack)
        offsets = np.zeros(n + 1, dtype=U32)
        np.cumsum(caps, out=offsets[1:])
        total = int(offsets[-1])
        keys = np.zeros(total, dtype=U64)
        actors = np.zeros(total, dtype=U32)
        counters = np.zeros(total, dtype=U64)
        vv = np.zeros(n * R, dtype=U64)
        for d, (ents, v) in enumerate(docs):
            o = int(offsets[d])
            for i, (k, a, c) in enumerate(ents):
                keys[o + i], actors[o + i], counters[o + i] = k, a, c
            vv[d * R:(d + 1) * R] = v
        return AWSetBatch(R, offsets, keys, actors, counters, vv, counts if slack else None)

    def live(self, d) -> int:
        if self.counts is not None:
            return int(self.counts[d])
        return int(self.offsets[d + 1]) - int(self.offsets[d])

    def doc(self, d):
        """(entries [(key, actor, counter)], vv list) of doc d (host batch)."""
        o, n = int(self.offsets[d]), self.live(d)
        ents = list(zip(self.keys[o:o + n].tolist(), self.actors[o:o + n].tolist(), self.counters[o:o + n].tolist()))
        return ents, self.vv[d * self.R:(d + 1) * self.R].tolist()

    def live_slots(self) -> int:
        if self.counts is not None:
            return int(np.asarray(_np(self.counts, U32), dtype=np.uint64).sum())
        o = _np(self.offsets, U32)
        return int(o[-1]) - int(o[0])


def pinned_zeros(n, dtype):
    """A zeroed numpy array in page-locked host memory (crdt_host_alloc), freed
    with the array.  The *_batch calls stage inputs that lie in one such block
    with one copy, and write packed outputs that lie in such blocks from the
    gather kernel (api.cpp, fetch_outputs)."""
    import weakref

    from . import abi

    lib = abi.lib()
    nbytes = max(int(n), 1) * np.dtype(dtype).itemsize
    p = ctypes.c_void_p()
    rc = lib.crdt_host_alloc(nbytes, ctypes.byref(p))
    if rc != 0:
        raise MemoryError("crdt_host_alloc(%d): %d" % (nbytes, rc))
    buf = (ctypes.c_char * nbytes).from_address(p.value)
    arr = np.frombuffer(buf, dtype=dtype, count=max(int(n), 1))
    arr[:] = 0
    weakref.finalize(buf, lib.crdt_host_free, ctypes.c_void_p(p.value))
    return arr


class OutBuffers:
    """Output of a join/fold: n_docs docs, `slots` capacity, numpy or torch.
    shared_keys: another OutBuffers whose key column this one uses (the two
    outputs of an exchange hold the same keys at the same slots,
    crdt_awset_exchange_async).  pinned: host arrays in page-locked memory."""

    def __init__(self, n_docs, R, slots, device=None, shared_keys=None, pinned=False):
        self.R, self.n_docs, self.slots = int(R), int(n_docs), int(slots)
        if device is None:
            z = pinned_zeros if pinned else (lambda n, dt: np.zeros(n, dtype=dt))
            self.offsets = z(n_docs + 1, U32)
            self.counts = z(n_docs, U32)[:n_docs]
            self.keys = z(max(slots, 1), U64)
            self.actors = z(max(slots, 1), U32)
            self.counters = z(max(slots, 1), U64)
            self.vv = z(max(n_docs * R, 1), U64)
        else:
            import torch

            e = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=device)  # noqa: E731
            self.offsets = e(n_docs + 1, torch.int32)[: n_docs + 1]
            self.counts = e(n_docs, torch.int32)[:n_docs]
            self.keys = e(slots if shared_keys is None else 0, torch.int64)
            self.actors = e(slots, torch.int32)
            self.counters = e(slots, torch.int64)
            self.vv = e(n_docs * R, torch.int64)
        if shared_keys is not None:
            assert shared_keys.slots >= self.slots
            self.keys = shared_keys.keys

    def c(self) -> CAWSetOut:
        return CAWSetOut(ptr(self.offsets), ptr(self.counts), ptr(self.keys), ptr(self.actors), ptr(self.counters),
                         ptr(self.vv))

    def as_batch(self) -> AWSetBatch:
        return AWSetBatch(self.R, self.offsets, self.keys, self.actors, self.counters, self.vv, counts=self.counts)


class SrcBatch:
    """Ordered sources folded into each doc (AWSet or AWSetDelta states)."""

    def __init__(self, R, doc_srcs, src_actor, vv, entry_off, keys, actors, counters,
                 tomb_off=None, tkeys=None, tactors=None, tcounters=None):
        self.R = int(R)
        self.doc_srcs, self.src_actor, self.vv, self.entry_off = doc_srcs, src_actor, vv, entry_off
        self.keys, self.actors, self.counters = keys, actors, counters
        self.tomb_off, self.tkeys, self.tactors, self.tcounters = tomb_off, tkeys, tactors, tcounters

    @property
    def n_docs(self) -> int:
        return int(self.doc_srcs.shape[0]) - 1

    @property
    def n_srcs(self) -> int:
        return int(self.src_actor.shape[0])

    def c(self) -> CSrcBatch:
        return CSrcBatch(self.n_docs, self.R, ptr(self.doc_srcs), ptr(self.src_actor), ptr(self.vv),
                         ptr(self.entry_off), ptr(self.keys), ptr(self.actors), ptr(self.counters),
                         ptr(self.tomb_off), ptr(self.tkeys), ptr(self.tactors), ptr(self.tcounters))

    def c_delta_out(self, kind=None) -> CDeltaOut:
        """These arrays as the message a delta extraction writes (crdt_delta_out)."""
        return CDeltaOut(ptr(self.doc_srcs), ptr(self.src_actor), ptr(self.vv), ptr(self.entry_off), ptr(self.keys),
                         ptr(self.actors), ptr(self.counters), ptr(self.tomb_off), ptr(self.tkeys),
                         ptr(self.tactors), ptr(self.tcounters), ptr(kind))

    _FIELDS = (("doc_srcs", U32), ("src_actor", U32), ("vv", U64), ("entry_off", U32), ("keys", U64),
               ("actors", U32), ("counters", U64), ("tomb_off", U32), ("tkeys", U64), ("tactors", U32),
               ("tcounters", U64))

    def to(self, device) -> "SrcBatch":
        return SrcBatch(self.R, *(_torch(getattr(self, f), device) for f, _ in self._FIELDS))

    def numpy(self) -> "SrcBatch":
        return SrcBatch(self.R, *(_np(getattr(self, f), dt) for f, dt in self._FIELDS))

    @staticmethod
    def from_lists(R, per_doc) -> "SrcBatch":
        """per_doc[d] = list of sources (actor, vv, entries [(k,a,c)], tombstones [(k,a,c)] or None)."""
        srcs = [s for lst in per_doc for s in lst]
        doc_srcs = np.zeros(len(per_doc) + 1, dtype=U32)
        np.cumsum([len(lst) for lst in per_doc], out=doc_srcs[1:])
        ns = len(srcs)
        src_actor = np.array([s[0] for s in srcs], dtype=U32).reshape(ns)
        vv = np.zeros(max(ns * R, 1), dtype=U64)
        entry_off = np.zeros(ns + 1, dtype=U32)
        tomb_off = np.zeros(ns + 1, dtype=U32)
        for i, s in enumerate(srcs):
            vv[i * R:(i + 1) * R] = s[1]
            entry_off[i + 1] = entry_off[i] + len(s[2])
            tomb_off[i + 1] = tomb_off[i] + len(s[3] or [])
        def flat(idx, off):
            n = int(off[-1])
            k, a, c = np.zeros(max(n, 1), U64), np.zeros(max(n, 1), U32), np.zeros(max(n, 1), U64)
            for i, s in enumerate(srcs):
                for j, (kk, aa, cc) in enumerate(s[idx] or []):
                    k[off[i] + j], a[off[i] + j], c[off[i] + j] = kk, aa, cc
            return k, a, c
        keys, actors, counters = flat(2, entry_off)
        tkeys, tactors, tcounters = flat(3, tomb_off)
        return SrcBatch(R, doc_srcs, src_actor, vv, entry_off, keys, actors, counters,
                        tomb_off, tkeys, tactors, tcounters)

    def out_slots(self, dst: AWSetBatch) -> int:
        eo = _np(self.entry_off, U32)
        return int(_np(dst.offsets, U32)[-1]) + int(eo[-1])


class SrcBuffers(SrcBatch):
    """Device (torch) or host (numpy) storage for n_srcs sources of fixed
    entry / tombstone slot counts (what the workload generators fill)."""

    def __init__(self, R, n_docs, n_srcs, entry_slots, tomb_slots, device=None):
        if device is None:
            z = lambda n, dt: np.zeros(max(n, 1), dtype=dt)  # noqa: E731
            i32, i64 = U32, U64
        else:
            import torch

            z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device=device)  # noqa: E731
            i32, i64 = torch.int32, torch.int64
        super().__init__(R, z(n_docs + 1, i32)[: n_docs + 1], z(n_srcs, i32)[:n_srcs], z(n_srcs * R, i64),
                         z(n_srcs + 1, i32)[: n_srcs + 1], z(entry_slots, i64), z(entry_slots, i32),
                         z(entry_slots, i64), z(n_srcs + 1, i32)[: n_srcs + 1], z(tomb_slots, i64),
                         z(tomb_slots, i32), z(tomb_slots, i64))


class OpBatch:
    """Per doc an ordered list of local ops (include/crdtgpu.h, CRDT_OP_*) and
    the doc's replica actor."""

    def __init__(self, op_off, kind, keys, doc_actor):
        self.op_off, self.kind, self.keys, self.doc_actor = op_off, kind, keys, doc_actor

    @property
    def n_docs(self) -> int:
        return int(self.op_off.shape[0]) - 1

    def c(self) -> COpBatch:
        return COpBatch(self.n_docs, ptr(self.op_off), ptr(self.kind), ptr(self.keys), ptr(self.doc_actor))

    def numpy(self) -> "OpBatch":
        return OpBatch(_np(self.op_off, U32), _np(self.kind, np.uint8), _np(self.keys, U64),
                       _np(self.doc_actor, U32))

    def to(self, device) -> "OpBatch":
        return OpBatch(*(_torch(a, device) for a in (self.op_off, self.kind, self.keys, self.doc_actor)))

    @staticmethod
    def from_lists(per_doc, actors) -> "OpBatch":
        """per_doc[d] = [(kind, key)], actors[d] = the doc's replica actor."""
        op_off = np.zeros(len(per_doc) + 1, dtype=U32)
        np.cumsum([len(x) for x in per_doc], out=op_off[1:])
        n = int(op_off[-1])
        kind = np.zeros(max(n, 1), dtype=np.uint8)
        keys = np.zeros(max(n, 1), dtype=U64)
        i = 0
        for lst in per_doc:
            for k, key in lst:
                kind[i], keys[i] = k, key
                i += 1
        return OpBatch(op_off, kind, keys, np.asarray(actors, dtype=U32).reshape(len(per_doc)))


class TombBatch:
    """AWSetDelta.Deleted of each doc: sorted (key, actor, counter) per doc."""

    def __init__(self, offsets, keys, actors, counters, counts=None):
        self.offsets, self.keys, self.actors, self.counters, self.counts = offsets, keys, actors, counters, counts

    @property
    def n_docs(self) -> int:
        return int(self.offsets.shape[0]) - 1

    def c(self) -> CTombBatch:
        return CTombBatch(ptr(self.offsets), ptr(self.counts), ptr(self.keys), ptr(self.actors), ptr(self.counters))

    def numpy(self) -> "TombBatch":
        return TombBatch(_np(self.offsets, U32), _np(self.keys, U64), _np(self.actors, U32), _np(self.counters, U64),
                         _np(self.counts, U32))

    def to(self, device) -> "TombBatch":
        return TombBatch(*(_torch(a, device) for a in (self.offsets, self.keys, self.actors, self.counters)),
                         counts=_torch(self.counts, device))

    @staticmethod
    def from_lists(per_doc) -> "TombBatch":
        offsets = np.zeros(len(per_doc) + 1, dtype=U32)
        np.cumsum([len(x) for x in per_doc], out=offsets[1:])
        n = int(offsets[-1])
        k, a, c = np.zeros(max(n, 1), U64), np.zeros(max(n, 1), U32), np.zeros(max(n, 1), U64)
        i = 0
        for lst in per_doc:
            for kk, aa, cc in lst:
                k[i], a[i], c[i] = kk, aa, cc
                i += 1
        return TombBatch(offsets, k, a, c)

    def doc(self, d):
        o = int(self.offsets[d])
        n = int(self.counts[d]) if self.counts is not None else int(self.offsets[d + 1]) - o
        return list(zip(self.keys[o:o + n].tolist(), self.actors[o:o + n].tolist(), self.counters[o:o + n].tolist()))


class TombBuffers(TombBatch):
    """Output tombstones of an apply call (numpy, or torch on `device`)."""

    def __init__(self, n_docs, slots, device=None):
        if device is None:
            super().__init__(np.zeros(n_docs + 1, U32), np.zeros(max(slots, 1), U64), np.zeros(max(slots, 1), U32),
                             np.zeros(max(slots, 1), U64), np.zeros(max(n_docs, 1), U32)[:n_docs])
        else:
            import torch

            e = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=device)  # noqa: E731
            super().__init__(e(n_docs + 1, torch.int32)[: n_docs + 1], e(slots, torch.int64), e(slots, torch.int32),
                             e(slots, torch.int64), e(n_docs, torch.int32)[:n_docs])

    def c_out(self) -> CTombOut:
        return CTombOut(ptr(self.offsets), ptr(self.counts), ptr(self.keys), ptr(self.actors), ptr(self.counters))


class Replica:
    """One resident replica of every document (crdt_replica): its state batch, its
    AWSetDelta.Deleted (tombs, None: none) and its actor -- doc_actor, a u32 per
    document as in OpBatch, or the scalar `actor` for every document."""

    def __init__(self, state: AWSetBatch, tombs: TombBatch = None, actor: int = 0, doc_actor=None):
        self.state, self.tombs, self.actor, self.doc_actor = state, tombs, int(actor), doc_actor

    @property
    def n_docs(self) -> int:
        return self.state.n_docs

    def c(self) -> CReplica:
        cs = self.state.c()
        ct = self.tombs.c() if self.tombs is not None else None
        r = CReplica(ctypes.addressof(cs), ctypes.addressof(ct) if ct is not None else None, ptr(self.doc_actor),
                     self.actor)
        r._keep = (cs, ct)  # the structs the descriptor points at live as long as it does
        return r

    def numpy(self) -> "Replica":
        return Replica(self.state.numpy(), self.tombs.numpy() if self.tombs is not None else None, self.actor,
                       _np(self.doc_actor, U32))

    def to(self, device) -> "Replica":
        return Replica(self.state.to(device), self.tombs.to(device) if self.tombs is not None else None,
                       self.actor, _torch(self.doc_actor, device))


class ReplicaBuffers:
    """Storage a replica select / scatter writes (crdt_replica_out): the state
    (OutBuffers of `entry_slots`), the tombstones (TombBuffers of `tomb_slots`;
    tombs=False: none, for replicas without a Deleted map) and the per-document
    actors (actors=False: not written).  numpy, or torch on `device`.
    as_replica() hands the result back as the Replica of the next call."""

    def __init__(self, n_docs, R, entry_slots, tomb_slots=0, device=None, tombs=True, actors=True):
        self.n_docs, self.R = int(n_docs), int(R)
        self.entry_slots, self.tomb_slots = int(entry_slots), int(tomb_slots) if tombs else 0
        self.state = OutBuffers(n_docs, R, entry_slots, device=device)
        self.tombs = TombBuffers(n_docs, tomb_slots, device=device) if tombs else None
        if not actors:
            self.doc_actor = None
        elif device is None:
            self.doc_actor = np.zeros(max(n_docs, 1), U32)[:n_docs]
        else:
            import torch

            self.doc_actor = torch.empty(max(n_docs, 1), dtype=torch.int32, device=device)[:n_docs]

    def c(self) -> CReplicaOut:
        cs = self.state.c()
        ct = self.tombs.c_out() if self.tombs is not None else None
        r = CReplicaOut(ctypes.addressof(cs), ctypes.addressof(ct) if ct is not None else None, ptr(self.doc_actor))
        r._keep = (cs, ct)  # the structs the descriptor points at live as long as it does
        return r

    def as_replica(self, actor: int = 0) -> "Replica":
        """The written replica as an input: its state with counts, its tombstones with
        counts, and its actors (`actor` for every document when they were not written)."""
        return Replica(self.state.as_batch(), self.tombs, actor, self.doc_actor)

    def numpy(self) -> "Replica":
        """Host copy trimmed to the packed totals (offsets[n_docs] of entries and tombstones,
        each at most its slots)."""
        n, R = self.n_docs, self.R
        off = _np(self.state.offsets, U32)[: n + 1]
        te = min(int(off[n]), self.entry_slots)
        st = AWSetBatch(R, off, _np(self.state.keys, U64)[:te], _np(self.state.actors, U32)[:te],
                        _np(self.state.counters, U64)[:te], _np(self.state.vv, U64)[: n * R],
                        counts=_np(self.state.counts, U32)[:n])
        tb = None
        if self.tombs is not None:
            toff = _np(self.tombs.offsets, U32)[: n + 1]
            tt = min(int(toff[n]), self.tomb_slots)
            tb = TombBatch(toff, _np(self.tombs.keys, U64)[:tt], _np(self.tombs.actors, U32)[:tt],
                           _np(self.tombs.counters, U64)[:tt], counts=_np(self.tombs.counts, U32)[:n])
        da = None if self.doc_actor is None else _np(self.doc_actor, U32)[:n]
        return Replica(st, tb, 0, da)


@dataclasses.dataclass(frozen=True)
class Headroom:
    """The layout policy of a replica repack (crdt_headroom): a document with n live
    slots owns round_up(n + max(min_spare, (n * num) >> shift), align) slots.  The
    default is packed.  The expression itself lives in the library
    (crdt_headroom_capacity), and capacity() asks it."""

    min_spare: int = 0
    num: int = 0
    shift: int = 0
    align: int = 1

    def c(self) -> CHeadroom:
        return CHeadroom(self.min_spare, self.num, self.shift, self.align)

    def capacity(self, n: int) -> int:
        from . import abi

        h = self.c()
        return int(abi.lib().crdt_headroom_capacity(ctypes.byref(h), int(n)))

    def total(self, counts) -> int:
        """Slots a repack asks for, for a host-known vector of live counts (one capacity
        per distinct count from the library; the sum is not saturated)."""
        vals, reps = np.unique(np.asarray(counts, U32), return_counts=True)
        return sum(self.capacity(int(v)) * int(r) for v, r in zip(vals, reps))


def repack_slots(entry_counts, tomb_counts=None, entry_room=None, tomb_room=None):
    """(entry_slots, tomb_slots) that crdt_replica_repack_async needs for output
    documents with these live counts (host arrays, one per output document; empty
    documents count with 0).  tomb_counts None: every document has no tombstone."""
    ec = np.asarray(entry_counts, U32)
    tc = np.zeros(len(ec), U32) if tomb_counts is None else np.asarray(tomb_counts, U32)
    return (entry_room or Headroom()).total(ec), (tomb_room or Headroom()).total(tc)


class InplaceTarget:
    """A resident replica as the target of an in-place scatter (crdt_replica_inplace):
    the state's arrays with its counts, the tombstones with theirs (None: the replica
    keeps no Deleted) and the per-document actors (None: not written).  The offsets
    are read, everything else is written where a document is placed.  of() views a
    Replica, a ReplicaBuffers or an OutBuffers (with a TombBuffers) as it stands."""

    def __init__(self, state, tombs=None, doc_actor=None):
        self.state, self.tombs, self.doc_actor = state, tombs, doc_actor
        if state.counts is None or (tombs is not None and tombs.counts is None):
            raise ValueError("an in-place target needs counts: a document's length changes")

    @staticmethod
    def of(x, tombs=None, doc_actor=None, actors=True) -> "InplaceTarget":
        if isinstance(x, InplaceTarget):
            return x
        if isinstance(x, (Replica, ReplicaBuffers)):
            st = x.state if isinstance(x.state, AWSetBatch) else x.state.as_batch()
            return InplaceTarget(st, x.tombs, x.doc_actor if actors else None)
        if isinstance(x, OutBuffers):
            return InplaceTarget(x.as_batch(), tombs, doc_actor)
        return InplaceTarget(x, tombs, doc_actor)  # an AWSetBatch with counts

    @property
    def n_docs(self) -> int:
        return self.state.n_docs

    def c(self) -> CReplicaInplace:
        s, t = self.state, self.tombs
        tp = [ptr(getattr(t, f)) for f in ("offsets", "counts", "keys", "actors", "counters")] if t is not None \
            else [None] * 5
        return CReplicaInplace(s.n_docs, s.R, ptr(s.offsets), ptr(s.counts), ptr(s.keys), ptr(s.actors),
                               ptr(s.counters), ptr(s.vv), *tp, ptr(self.doc_actor))

    def as_replica(self, actor: int = 0) -> "Replica":
        return Replica(self.state, self.tombs, actor, self.doc_actor)


class SpillBuffers:
    """The lists an in-place scatter writes (crdt_spill_out): the sub documents that
    did not fit, ascending (spill_j), the replica document each names (spill_doc) and
    their number (n_spill, one word); n_sub words each.  numpy, or torch on `device`.
    spill_j / n_spill are the idx / n_idx of the select, spill_doc / n_spill those of
    the scatter, that put the spilled documents back."""

    def __init__(self, n_sub, device=None):
        self.n_sub = int(n_sub)
        if device is None:
            self.spill_j, self.spill_doc = (np.zeros(max(n_sub, 1), U32) for _ in range(2))
            self.n_spill = np.zeros(1, U32)
        else:
            import torch

            self.spill_j, self.spill_doc = (torch.empty(max(n_sub, 1), dtype=torch.int32, device=device)
                                            for _ in range(2))
            self.n_spill = torch.empty(1, dtype=torch.int32, device=device)

    def c(self) -> CSpillOut:
        return CSpillOut(ptr(self.spill_j), ptr(self.spill_doc), ptr(self.n_spill))

    def numpy(self):
        """(spill_j, spill_doc) trimmed to *n_spill."""
        n = int(_np(self.n_spill, U32)[0])
        return _np(self.spill_j, U32)[:n].copy(), _np(self.spill_doc, U32)[:n].copy()


class DigestTreeBuffers:
    """The digest tree over a digest array of n_docs docs (crdt_digest_tree_async) and the
    buffers of a descent over it: `tree` (u64, two words per node, levels 1 .. L
    concatenated), and for lists of up to `cap` nodes or docs per level the packed children
    (`packed`, 32 words per listed parent), two list / count pairs used in turn (`idx`,
    `n_out`), the last level's `flags` and `summary`.  cap None: no descent buffers.
    numpy, or torch on `device`.  L, nodes[l] and off[l] are the layout
    (crdt_digest_tree_layout)."""

    def __init__(self, n_docs, device=None, cap=None):
        from .abi import lib

        self.n_docs = int(n_docs)
        nodes, off = np.zeros(9, U32), np.zeros(9, U32)
        self.L = int(lib().crdt_digest_tree_layout(self.n_docs, nodes.ctypes.data, off.ctypes.data))
        self.nodes, self.off = [int(x) for x in nodes], [int(x) for x in off]
        self.n_nodes = self.off[self.L] + 1 if self.L else 0
        self.cap = None if cap is None else max(int(cap), 16)  # (16: the root's children)
        if device is None:
            e = lambda k, dt: np.zeros(max(k, 1), dt)  # noqa: E731
            u64, u32, u8 = np.uint64, U32, np.uint8
        else:
            import torch

            e = lambda k, dt: torch.zeros(max(k, 1), dtype=dt, device=device)  # noqa: E731
            u64, u32, u8 = torch.int64, torch.int32, torch.uint8
        self.tree = e(2 * self.n_nodes, u64)
        if self.cap is not None:
            self.packed = e(32 * self.cap, u64)
            self.idx = [e(self.cap, u32), e(self.cap, u32)]
            self.n_out = [e(1, u32), e(1, u32)]
            self.flags = e(self.cap, u8)
            self.summary = e(5, u32)

    def level(self, l, digest):
        """(node array of level l, its node count): the digest array at l == 0."""
        if l == 0:
            return digest, self.n_docs
        return self.tree[2 * self.off[l]: 2 * (self.off[l] + self.nodes[l])], self.nodes[l]


class QueryBatch:
    """Per doc a list of query keys (crdt_query_batch): doc d asks
    keys[q_off[d]:q_off[d+1]], in any order, duplicates allowed."""

    def __init__(self, q_off, keys, n_queries=None):
        self.q_off, self.keys = q_off, keys
        # host-known (crdt_query_batch.n_queries): read once here, never from a device q_off later
        self.n_queries = int(_np(q_off, U32)[-1]) if n_queries is None else int(n_queries)

    @property
    def n_docs(self) -> int:
        return int(self.q_off.shape[0]) - 1

    def c(self) -> CQueryBatch:
        return CQueryBatch(self.n_docs, self.n_queries, ptr(self.q_off), ptr(self.keys))

    def numpy(self) -> "QueryBatch":
        return QueryBatch(_np(self.q_off, U32), _np(self.keys, U64), self.n_queries)

    def to(self, device) -> "QueryBatch":
        return QueryBatch(_torch(self.q_off, device), _torch(self.keys, device), self.n_queries)

    @staticmethod
    def from_lists(per_doc_keys) -> "QueryBatch":
        q_off = np.zeros(len(per_doc_keys) + 1, dtype=U32)
        np.cumsum([len(x) for x in per_doc_keys], out=q_off[1:])
        n = int(q_off[-1])
        keys = np.zeros(max(n, 1), dtype=U64)
        if n:
            keys[:n] = np.concatenate([np.asarray(x, dtype=U64) for x in per_doc_keys if len(x)])
        return QueryBatch(q_off, keys, n)


class QueryBuffers:
    """Outputs of a membership read (crdt_query_out), one per query: found (u8)
    and, with dots, the entry's actor and counter.  numpy, or torch on `device`."""

    def __init__(self, n_queries, device=None, dots=True):
        self.n_queries = n = int(n_queries)
        if device is None:
            self.found = np.zeros(max(n, 1), np.uint8)
            self.actors = np.zeros(max(n, 1), U32) if dots else None
            self.counters = np.zeros(max(n, 1), U64) if dots else None
        else:
            import torch

            e = lambda dt: torch.empty(max(n, 1), dtype=dt, device=device)  # noqa: E731
            self.found = e(torch.uint8)
            self.actors = e(torch.int32) if dots else None
            self.counters = e(torch.int64) if dots else None

    def c(self) -> CQueryOut:
        return CQueryOut(ptr(self.found), ptr(self.actors), ptr(self.counters))

    def numpy(self):
        """(found, actors, counters) as numpy arrays of n_queries (dots absent: None)."""
        n = self.n_queries
        f = lambda a, dt: None if a is None else _np(a, dt)[:n]  # noqa: E731
        return f(self.found, np.uint8), f(self.actors, U32), f(self.counters, U64)


class CompareBuffers:
    """Outputs of a convergence check (crdt_compare_out): flags (u8 per doc, OR of
    CRDT_CMP_*), summary (5 counts), worklist (ascending ids of the docs with
    flags & mask) and n_work (its length, one word -- on the device it feeds
    select_async as n_idx with no read-back).  numpy, or torch on `device`."""

    def __init__(self, n_docs, device=None, worklist=True, summary=True):
        self.n_docs = n = int(n_docs)
        if device is None:
            self.flags = np.zeros(max(n, 1), np.uint8)
            self.summary = np.zeros(5, U32) if summary else None
            self.worklist = np.zeros(max(n, 1), U32) if worklist else None
            self.n_work = np.zeros(1, U32) if worklist else None
        else:
            import torch

            e = lambda k, dt: torch.empty(max(k, 1), dtype=dt, device=device)  # noqa: E731
            self.flags = e(n, torch.uint8)
            self.summary = e(5, torch.int32) if summary else None
            self.worklist = e(n, torch.int32) if worklist else None
            self.n_work = e(1, torch.int32) if worklist else None

    def c(self) -> CCompareOut:
        return CCompareOut(ptr(self.flags), ptr(self.summary), ptr(self.worklist), ptr(self.n_work))

    def numpy(self):
        """(flags [n_docs], summary [5] or None, worklist [n_work] or None) as numpy arrays."""
        flags = _np(self.flags, np.uint8)[: self.n_docs]
        summary = None if self.summary is None else _np(self.summary, U32)
        if self.worklist is None:
            return flags, summary, None
        nw = int(_np(self.n_work, U32)[0])
        return flags, summary, _np(self.worklist, U32)[:nw]


class DiffBuffers:
    """Outputs of a merge diff (crdt_diff_out): flags (u8 per doc, OR of CRDT_DIFF_*),
    summary (5 counts), and the two packed lists with their [n_docs + 1] exclusive
    offsets: removed (rem_off, rem_keys, rem_actors, rem_counters; rem_slots entries of
    room) and upserted (ups_off, ups_keys, ups_actors, ups_counters, ups_kind; ups_slots).
    dots / kind False: those columns are not asked for.  numpy, or torch on `device`."""

    def __init__(self, n_docs, rem_slots, ups_slots, device=None, dots=True, kind=True, summary=True):
        self.n_docs = n = int(n_docs)
        self.rem_slots, self.ups_slots = nr, nu = int(rem_slots), int(ups_slots)
        if device is None:
            z = lambda k, dt: np.zeros(max(k, 1), dt)  # noqa: E731
            u8, u32, u64 = np.uint8, U32, U64
        else:
            import torch

            z = lambda k, dt: torch.empty(max(k, 1), dtype=dt, device=device)  # noqa: E731
            u8, u32, u64 = torch.uint8, torch.int32, torch.int64
        self.flags = z(n, u8)
        self.summary = z(5, u32) if summary else None
        self.rem_off, self.ups_off = z(n + 1, u32), z(n + 1, u32)
        self.rem_keys, self.ups_keys = z(nr, u64), z(nu, u64)
        self.rem_actors = z(nr, u32) if dots else None
        self.rem_counters = z(nr, u64) if dots else None
        self.ups_actors = z(nu, u32) if dots else None
        self.ups_counters = z(nu, u64) if dots else None
        self.ups_kind = z(nu, u8) if kind else None

    FIELDS = ("flags", "summary", "rem_off", "rem_keys", "rem_actors", "rem_counters", "ups_off", "ups_keys",
              "ups_actors", "ups_counters", "ups_kind")

    def c(self) -> CDiffOut:
        return CDiffOut(*(ptr(getattr(self, f)) for f in self.FIELDS))

    def numpy(self):
        """A dict of numpy arrays: flags [n_docs], summary [5] or None, the offsets
        [n_docs + 1], and each list's columns trimmed to min(total, slots) (absent: None)."""
        n = self.n_docs
        out = {"flags": _np(self.flags, np.uint8)[:n],
               "summary": None if self.summary is None else _np(self.summary, U32)[:5]}
        for side, slots in (("rem", self.rem_slots), ("ups", self.ups_slots)):
            off = _np(getattr(self, side + "_off"), U32)[: n + 1]
            m = min(int(off[n]), slots)
            out[side + "_off"] = off
            for col, dt in (("keys", U64), ("actors", U32), ("counters", U64)):
                a = getattr(self, "%s_%s" % (side, col))
                out["%s_%s" % (side, col)] = None if a is None else _np(a, dt)[:m]
            if side == "ups":
                out["ups_kind"] = None if self.ups_kind is None else _np(self.ups_kind, np.uint8)[:m]
        return out


class MergeLogBuffers:
    """The log a logged join writes beside the merged state (crdt_merge_log): flags (u8
    per doc, OR of CRDT_DIFF_*), summary (5 counts), and the two lists in the inputs' own
    slot layouts -- removed in dst's (rem_offsets = dst.offsets, rem_counts, rem_keys,
    rem_actors, rem_counters; rem_slots = dst's slots) and upserted in src's (ups_offsets,
    ups_counts, ups_keys, ups_actors, ups_counters, ups_kind; ups_slots = src's slots).
    kind / summary False: not asked for.  numpy, or torch on `device`."""

    def __init__(self, n_docs, rem_slots, ups_slots, device=None, kind=True, summary=True):
        self.n_docs = n = int(n_docs)
        self.rem_slots, self.ups_slots = nr, nu = int(rem_slots), int(ups_slots)
        if device is None:
            z = lambda k, dt: np.zeros(max(k, 1), dt)  # noqa: E731
            u8, u32, u64 = np.uint8, U32, U64
        else:
            import torch

            z = lambda k, dt: torch.empty(max(k, 1), dtype=dt, device=device)  # noqa: E731
            u8, u32, u64 = torch.uint8, torch.int32, torch.int64
        self.flags = z(n, u8)
        self.summary = z(5, u32) if summary else None
        self.rem_offsets, self.ups_offsets = z(n + 1, u32), z(n + 1, u32)
        self.rem_counts, self.ups_counts = z(n, u32), z(n, u32)
        self.rem_keys, self.rem_actors, self.rem_counters = z(nr, u64), z(nr, u32), z(nr, u64)
        self.ups_keys, self.ups_actors, self.ups_counters = z(nu, u64), z(nu, u32), z(nu, u64)
        self.ups_kind = z(nu, u8) if kind else None

    FIELDS = ("flags", "summary", "rem_offsets", "rem_counts", "rem_keys", "rem_actors", "rem_counters",
              "ups_offsets", "ups_counts", "ups_keys", "ups_actors", "ups_counters", "ups_kind")
    _DTYPES = (np.uint8, U32, U32, U32, U64, U32, U64, U32, U32, U64, U32, U64, np.uint8)

    def c(self) -> CMergeLog:
        return CMergeLog(*(ptr(getattr(self, f)) for f in self.FIELDS))

    def removed(self) -> "TombBatch":
        """The removed list as a TombBatch as it stands (offsets, counts and the three columns)."""
        return TombBatch(self.rem_offsets[: self.n_docs + 1], self.rem_keys, self.rem_actors, self.rem_counters,
                         counts=self.rem_counts[: self.n_docs])

    def upserted(self) -> "TombBatch":
        """The upserted list as a TombBatch as it stands."""
        return TombBatch(self.ups_offsets[: self.n_docs + 1], self.ups_keys, self.ups_actors, self.ups_counters,
                         counts=self.ups_counts[: self.n_docs])

    def numpy(self):
        """A dict of numpy arrays, one per field (absent: None): flags [n_docs], summary [5],
        the offsets [n_docs + 1], the counts [n_docs] and the columns at their full slots."""
        n = self.n_docs
        size = {"flags": n, "summary": 5, "rem_offsets": n + 1, "ups_offsets": n + 1, "rem_counts": n, "ups_counts": n}
        out = {}
        for f, dt in zip(self.FIELDS, self._DTYPES):
            a = getattr(self, f)
            if a is None:
                out[f] = None
                continue
            m = size.get(f, self.rem_slots if f.startswith("rem") else self.ups_slots)
            out[f] = _np(a, dt)[:m]
        return out


def c_ref(x):
    return ctypes.byref(x)
