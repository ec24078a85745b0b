"""Engine: one crdt_ctx (one per host thread), the batched merge entry points."""

from __future__ import annotations

import ctypes

from . import abi
from .abi import check
from .batch import (AWSetBatch, CompareBuffers, DiffBuffers, DigestTreeBuffers, Headroom, InplaceTarget, MergeLogBuffers, OpBatch, OutBuffers, QueryBatch, QueryBuffers, Replica, ReplicaBuffers, SpillBuffers, SrcBatch, SrcBuffers, TombBatch,
                    TombBuffers, _np, ptr)


def _c(x):
    """ctypes struct of a batch/output (or the struct itself, prebuilt by the caller
    to keep per-launch host work at a few ctypes calls)."""
    return x.c() if hasattr(x, "c") else x


def _stream(stream):
    if stream is None:
        return None
    if hasattr(stream, "cuda_stream"):
        return stream.cuda_stream
    return int(stream)


class Engine:
    def __init__(self, device: int = 0):
        self._lib = abi.lib()
        h = ctypes.c_void_p()
        check(self._lib.crdt_ctx_create(int(device), ctypes.byref(h)), "crdt_ctx_create")
        self._ctx = h
        self.device = device

    def close(self):
        if self._ctx:
            self._lib.crdt_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- workspace / errors ------------------------------------------------
    def reserve(self, max_docs: int, max_fold_slots: int = 0):
        check(self._lib.crdt_ctx_reserve(self._ctx, int(max_docs), int(max_fold_slots)), "crdt_ctx_reserve")

    def set_max_doc_entries(self, n: int = 0xFFFFFFFF):
        check(self._lib.crdt_ctx_set_max_doc_entries(self._ctx, int(n)), "crdt_ctx_set_max_doc_entries")

    def set_option(self, name: str, value: int):
        check(self._lib.crdt_ctx_set_option(self._ctx, name.encode(), int(value)), "crdt_ctx_set_option")

    def sync(self, stream=None):
        check(self._lib.crdt_ctx_sync(self._ctx, _stream(stream)), "crdt_ctx_sync")

    def clock_probe(self) -> float:
        """Shader clock in MHz under an all-CU integer load (crdt_clock_probe)."""
        g = ctypes.c_double()
        check(self._lib.crdt_clock_probe(self._ctx, ctypes.byref(g)), "crdt_clock_probe")
        return g.value

    def bw_probe(self, kind: int, a, b, nbytes: int, reps: int = 10) -> float:
        """GB/s of a streaming read / write / copy over device buffers a, b (crdt_bw_probe)."""
        g = ctypes.c_double()
        pa = a.data_ptr() if a is not None else None
        check(self._lib.crdt_bw_probe(self._ctx, int(kind), pa, b.data_ptr(), int(nbytes), int(reps), ctypes.byref(g)),
              "crdt_bw_probe")
        return g.value

    # -- device-resident, asynchronous -------------------------------------
    def join_async(self, dst: AWSetBatch, src: AWSetBatch, out: OutBuffers, stream=None):
        d, s, o = _c(dst), _c(src), _c(out)
        check(self._lib.crdt_awset_join_async(self._ctx, ctypes.byref(d), ctypes.byref(s), ctypes.byref(o),
                                              _stream(stream)), "crdt_awset_join_async")

    def exchange_async(self, a: AWSetBatch, b: AWSetBatch, out_ab: OutBuffers, out_ba: OutBuffers, stream=None):
        ca, cb, o1, o2 = _c(a), _c(b), _c(out_ab), _c(out_ba)
        check(self._lib.crdt_awset_exchange_async(self._ctx, ctypes.byref(ca), ctypes.byref(cb), ctypes.byref(o1),
                                                  ctypes.byref(o2), _stream(stream)), "crdt_awset_exchange_async")

    def fold_async(self, mode: int, dst: AWSetBatch, srcs: SrcBatch, out: OutBuffers, stream=None):
        d, s, o = _c(dst), _c(srcs), _c(out)
        check(self._lib.crdt_awset_fold_async(self._ctx, int(mode), ctypes.byref(d), ctypes.byref(s),
                                              ctypes.byref(o), _stream(stream)), "crdt_awset_fold_async")

    def delta_extract_async(self, srcs: SrcBatch, peer_vv, out: SrcBuffers, kind=None, stream=None):
        """Send side of anti-entropy: per doc, what a peer that has reached clock
        peer_vv[d*R..] still needs of each AWSetDelta source, packed into `out`
        (crdt_awset_delta_extract_async); kind: u8 per source, CRDT_DELTA_*."""
        s, o = _c(srcs), out.c_delta_out(kind)
        check(self._lib.crdt_awset_delta_extract_async(self._ctx, ctypes.byref(s), ptr(peer_vv), ctypes.byref(o),
                                                       _stream(stream)), "crdt_awset_delta_extract_async")

    def vv_max_async(self, dst, src, n: int, stream=None):
        check(self._lib.crdt_vv_max_async(self._ctx, ptr(dst), ptr(src), int(n), _stream(stream)),
              "crdt_vv_max_async")

    def causal_context_async(self, vv, n_docs: int, R: int, out, stream=None):
        check(self._lib.crdt_causal_context_async(self._ctx, ptr(vv), int(n_docs), int(R), ptr(out),
                                                  _stream(stream)), "crdt_causal_context_async")

    def apply_async(self, state: AWSetBatch, ops: OpBatch, out: OutBuffers, tombs: TombBatch = None,
                    tomb_out: TombBuffers = None, stream=None):
        """Device-resident batched Add / Del / AWSetDelta.Del (crdt_awset_apply_async)."""
        cs, co, cout = _c(state), _c(ops), _c(out)
        ct = _c(tombs) if tombs is not None else None
        cto = tomb_out.c_out() if tomb_out is not None else None
        check(self._lib.crdt_awset_apply_async(self._ctx, ctypes.byref(cs), ctypes.byref(ct) if ct else None,
                                               ctypes.byref(co), ctypes.byref(cout),
                                               ctypes.byref(cto) if cto else None, _stream(stream)),
              "crdt_awset_apply_async")

    def sort_async(self, batch: AWSetBatch, n_slots: int, out: OutBuffers, stream=None):
        """Ingest sort: each doc's live entries ordered by key (crdt_awset_sort_async)."""
        cb, co = _c(batch), _c(out)
        check(self._lib.crdt_awset_sort_async(self._ctx, ctypes.byref(cb), int(n_slots), ctypes.byref(co),
                                              _stream(stream)), "crdt_awset_sort_async")

    def sort(self, batch: AWSetBatch) -> OutBuffers:
        """Host buffers: the batch with each doc's live entries sorted by key."""
        b = batch.numpy()
        out = OutBuffers(b.n_docs, b.R, int(b.offsets[-1]))
        cb, co = b.c(), out.c()
        check(self._lib.crdt_awset_sort_batch(self._ctx, ctypes.byref(cb), ctypes.byref(co)), "crdt_awset_sort_batch")
        return out

    def tombstone_gc_async(self, tombs: TombBatch, R: int, stable_vv, out: TombBuffers, stream=None):
        """Opt-in GC: drop each doc's tombstones its stable clock covers (crdt_tombstone_gc_async)."""
        ct, co = _c(tombs), out.c_out()
        check(self._lib.crdt_tombstone_gc_async(self._ctx, ctypes.byref(ct), tombs.n_docs, int(R), ptr(stable_vv),
                                                ctypes.byref(co), _stream(stream)), "crdt_tombstone_gc_async")

    def has_async(self, state: AWSetBatch, queries: QueryBatch, out: QueryBuffers, stream=None):
        """(*AWSet).Has for each doc's query keys on a device-resident state, with the
        entry's dot (crdt_awset_has_async); a join / fold / apply output's as_batch() is a state."""
        s, q, o = _c(state), _c(queries), _c(out)
        check(self._lib.crdt_awset_has_async(self._ctx, ctypes.byref(s), ctypes.byref(q), ctypes.byref(o),
                                             _stream(stream)), "crdt_awset_has_async")

    def tomb_has_async(self, tombs: TombBatch, queries: QueryBatch, out: QueryBuffers, stream=None):
        """The same lookup over each doc's AWSetDelta.Deleted (crdt_tomb_has_async)."""
        t, q, o = _c(tombs), _c(queries), _c(out)
        check(self._lib.crdt_tomb_has_async(self._ctx, ctypes.byref(t), tombs.n_docs, ctypes.byref(q),
                                            ctypes.byref(o), _stream(stream)), "crdt_tomb_has_async")

    def compare_async(self, a: AWSetBatch, b: AWSetBatch, out: CompareBuffers, mask: int = 15, stream=None):
        """Per doc, CRDT_CMP_* of a[d] against b[d] (element sets, dots, clocks), the summary
        counts and the ascending worklist of docs with flags & mask (crdt_awset_compare_async)."""
        ca, cb, co = _c(a), _c(b), _c(out)
        check(self._lib.crdt_awset_compare_async(self._ctx, ctypes.byref(ca), ctypes.byref(cb), int(mask),
                                                 ctypes.byref(co), _stream(stream)), "crdt_awset_compare_async")

    def diff_async(self, before: AWSetBatch, after: AWSetBatch, out: DiffBuffers, rem_slots=None, ups_slots=None,
                   stream=None):
        """Per doc, what turns before[d] into after[d]: the removed entries and the upserted
        ones (ADDED / UPDATED), each list packed in key order behind exclusive offsets, and
        CRDT_DIFF_* flags (crdt_awset_diff_async).  A total above out's rem_slots / ups_slots:
        CRDT_E_CAPACITY at sync, offsets and totals exact, nothing written past the slots.
        The slot limits default to the sizes out was made with."""
        cb, ca, co = _c(before), _c(after), _c(out)
        rem_slots = out.rem_slots if rem_slots is None else rem_slots
        ups_slots = out.ups_slots if ups_slots is None else ups_slots
        check(self._lib.crdt_awset_diff_async(self._ctx, ctypes.byref(cb), ctypes.byref(ca), int(rem_slots),
                                              int(ups_slots), ctypes.byref(co), _stream(stream)),
              "crdt_awset_diff_async")

    def join_log_async(self, dst: AWSetBatch, src: AWSetBatch, out: OutBuffers, log: MergeLogBuffers, stream=None):
        """join_async with the merge's log written beside the merged state: per doc, the dst
        entries removed (in dst's slot layout) and the src entries added or moved to (in src's),
        with CRDT_DIFF_* flags and the summary -- what diff_async(dst, out) reports, from the
        one read the merge needs (crdt_awset_join_log_async)."""
        d, s, o, lg = _c(dst), _c(src), _c(out), _c(log)
        check(self._lib.crdt_awset_join_log_async(self._ctx, ctypes.byref(d), ctypes.byref(s), ctypes.byref(o),
                                                  ctypes.byref(lg), _stream(stream)), "crdt_awset_join_log_async")

    def exchange_log_async(self, a: AWSetBatch, b: AWSetBatch, out_ab: OutBuffers, out_ba: OutBuffers,
                           log_ab: MergeLogBuffers, log_ba: MergeLogBuffers, stream=None):
        """exchange_async with both directions' logs, from one read of both states: log_ab
        removed in a's layout and upserted in b's, log_ba the other way round.  The two outputs
        share no array, the key column included (crdt_awset_exchange_log_async)."""
        ca, cb, o1, o2, l1, l2 = _c(a), _c(b), _c(out_ab), _c(out_ba), _c(log_ab), _c(log_ba)
        check(self._lib.crdt_awset_exchange_log_async(self._ctx, ctypes.byref(ca), ctypes.byref(cb), ctypes.byref(o1),
                                                      ctypes.byref(o2), ctypes.byref(l1), ctypes.byref(l2),
                                                      _stream(stream)), "crdt_awset_exchange_log_async")

    def join_log(self, dst: AWSetBatch, src: AWSetBatch):
        """Host batches uploaded, merged with the log on the device and downloaded: (the
        merged state as host OutBuffers, MergeLogBuffers.numpy() of the log) (for tests and
        small callers)."""
        import numpy as np
        import torch

        dst, src = dst.numpy(), src.numpy()
        n, R = dst.n_docs, dst.R
        ds, ss = int(dst.offsets[-1]), int(src.offsets[-1])
        dev = torch.device("cuda", self.device)
        out = OutBuffers(n, R, ds + ss, device=dev)
        log = MergeLogBuffers(n, ds, ss, device=dev)
        self.join_log_async(dst.to(dev), src.to(dev), out, log)
        self.sync()
        h = OutBuffers(n, R, ds + ss)
        h.offsets, h.counts, h.vv = _np(out.offsets, np.uint32), _np(out.counts, np.uint32), _np(out.vv, np.uint64)
        h.keys, h.actors, h.counters = _np(out.keys, np.uint64), _np(out.actors, np.uint32), _np(out.counters, np.uint64)
        return h, log.numpy()

    def fold_log_async(self, mode: int, dst: AWSetBatch, srcs: SrcBatch, out: OutBuffers, log: MergeLogBuffers,
                       stream=None):
        """fold_async with the log of the whole ordered fold beside the merged state: per doc,
        the dst entries that are gone at the end (at dst.offsets[d]) and the entries that are
        new or under another dot at the end (at entry_off[doc_srcs[d]], capacity the sources'
        entry slots) -- what diff_async(dst, out) reports; steps in between do not show
        (crdt_awset_fold_log_async)."""
        d, s, o, lg = _c(dst), _c(srcs), _c(out), _c(log)
        check(self._lib.crdt_awset_fold_log_async(self._ctx, int(mode), ctypes.byref(d), ctypes.byref(s),
                                                  ctypes.byref(o), ctypes.byref(lg), _stream(stream)),
              "crdt_awset_fold_log_async")

    def fold_log(self, mode: int, dst: AWSetBatch, srcs: SrcBatch):
        """Host batches uploaded, folded with the log on the device and downloaded: (the merged
        state as host OutBuffers, the log as host MergeLogBuffers), both sized from the inputs
        (for tests and small callers)."""
        import numpy as np
        import torch

        dst, srcs = dst.numpy(), srcs.numpy()
        n, R = dst.n_docs, dst.R
        ds, es = int(dst.offsets[-1]), int(srcs.entry_off[-1])
        dev = torch.device("cuda", self.device)
        out = OutBuffers(n, R, ds + es, device=dev)
        log = MergeLogBuffers(n, ds, es, device=dev)
        self.reserve(n, ds + es)
        self.fold_log_async(mode, dst.to(dev), srcs.to(dev), out, log)
        self.sync()
        h = OutBuffers(n, R, ds + es)
        h.offsets, h.counts, h.vv = _np(out.offsets, np.uint32), _np(out.counts, np.uint32), _np(out.vv, np.uint64)
        h.keys, h.actors, h.counters = _np(out.keys, np.uint64), _np(out.actors, np.uint32), _np(out.counters, np.uint64)
        hl = MergeLogBuffers(n, ds, es)
        for f, a in log.numpy().items():
            setattr(hl, f, a)
        return h, hl

    def apply_log_async(self, state: AWSetBatch, ops: OpBatch, out: OutBuffers, log: MergeLogBuffers,
                        tombs: TombBatch = None, tomb_out: TombBuffers = None, stream=None):
        """apply_async with the log of what the ops changed beside the new state: per doc, the
        state entries removed (at state.offsets[d], with the dot they had) and the entries an
        ADD left new or under another dot (at op_off[d], capacity the doc's ops) -- what
        diff_async(state, out) reports; tombstone changes are not part of it, a refused doc's
        log is empty (crdt_awset_apply_log_async)."""
        cs, co, cout, lg = _c(state), _c(ops), _c(out), _c(log)
        ct = _c(tombs) if tombs is not None else None
        cto = tomb_out.c_out() if tomb_out is not None else None
        check(self._lib.crdt_awset_apply_log_async(self._ctx, ctypes.byref(cs), ctypes.byref(ct) if ct else None,
                                                   ctypes.byref(co), ctypes.byref(cout),
                                                   ctypes.byref(cto) if cto else None, ctypes.byref(lg),
                                                   _stream(stream)), "crdt_awset_apply_log_async")

    def apply_log(self, state: AWSetBatch, ops: OpBatch, tombs: TombBatch = None, with_tombs: bool = True):
        """Host batches uploaded, the ops applied with the log on the device and downloaded:
        (entries out, tombstones out or None, the log as host MergeLogBuffers), the first two as
        apply returns them (for tests and small callers)."""
        import numpy as np
        import torch

        state, ops = state.numpy(), ops.numpy()
        tombs = tombs.numpy() if tombs is not None else None
        n, R = state.n_docs, state.R
        ss, nops = int(state.offsets[-1]), int(ops.op_off[-1])
        ts = (int(tombs.offsets[-1]) if tombs is not None else 0) + nops
        dev = torch.device("cuda", self.device)
        out = OutBuffers(n, R, ss + nops, device=dev)
        tout = TombBuffers(n, ts, device=dev) if with_tombs else None
        log = MergeLogBuffers(n, ss, nops, device=dev)
        self.apply_log_async(state.to(dev), ops.to(dev), out, log, tombs.to(dev) if tombs is not None else None, tout)
        self.sync()
        h = OutBuffers(n, R, ss + nops)
        h.offsets, h.counts, h.vv = _np(out.offsets, np.uint32), _np(out.counts, np.uint32), _np(out.vv, np.uint64)
        h.keys, h.actors, h.counters = _np(out.keys, np.uint64), _np(out.actors, np.uint32), _np(out.counters, np.uint64)
        ht = None
        if with_tombs:
            ht = TombBuffers(n, ts)
            ht.offsets, ht.counts = _np(tout.offsets, np.uint32), _np(tout.counts, np.uint32)
            ht.keys, ht.actors, ht.counters = (_np(tout.keys, np.uint64), _np(tout.actors, np.uint32),
                                               _np(tout.counters, np.uint64))
        hl = MergeLogBuffers(n, ss, nops)
        for f, a in log.numpy().items():
            setattr(hl, f, a)
        return h, ht, hl

    def digest_async(self, state: AWSetBatch, out, tombs: TombBatch = None, stream=None):
        """Per doc, the 16-byte digest of its live state into `out` (device u64 [2 * n_docs]):
        word 0 the element set, word 1 elements, dots, Deleted and clock
        (crdt_awset_digest_async); a join / fold / apply output's as_batch() is a state."""
        s = _c(state)
        t = _c(tombs) if tombs is not None else None
        check(self._lib.crdt_awset_digest_async(self._ctx, ctypes.byref(s), ctypes.byref(t) if t else None, ptr(out),
                                                _stream(stream)), "crdt_awset_digest_async")

    def digest(self, state: AWSetBatch, tombs: TombBatch = None):
        """Host batch uploaded and digested on the device: numpy u64 [n_docs, 2] (for tests
        and small callers: a caller who holds host data uses digest_host)."""
        import numpy as np
        import torch

        dev = torch.device("cuda", self.device)
        state = state.numpy()
        out = torch.empty(max(2 * state.n_docs, 1), dtype=torch.int64, device=dev)
        ds, dt = state.to(dev), tombs.numpy().to(dev) if tombs is not None else None
        self.digest_async(ds, out, dt)
        self.sync()
        return _np(out, np.uint64)[: 2 * state.n_docs].reshape(state.n_docs, 2)

    def digest_idx_async(self, state: AWSetBatch, idx, digest, tombs: TombBatch = None, n_idx=None, n_max=None,
                         mode: int = abi.CRDT_DIGEST_GATHER, stream=None):
        """The digests of the listed docs only, written into `digest` (device u64, two words
        per doc of the replica) at their own positions; every other word keeps its bits
        (crdt_awset_digest_idx_async).  GATHER: state is the replica, doc idx[j] is digested.
        PLACE: state is a sub-batch whose doc j is the replica's doc idx[j].  idx / n_idx:
        device u32 arrays (a worklist / n_work); n_idx None: n_max; n_max None: len(idx)."""
        s = _c(state)
        t = _c(tombs) if tombs is not None else None
        n_max = int(idx.shape[0]) if n_max is None else int(n_max)
        n_digest = int(digest.shape[0]) // 2  # (GATHER: the call refuses an array that is not the replica's length)
        check(self._lib.crdt_awset_digest_idx_async(self._ctx, ctypes.byref(s), ctypes.byref(t) if t else None,
                                                    ptr(idx), ptr(n_idx), n_max, n_digest, int(mode), ptr(digest),
                                                    _stream(stream)), "crdt_awset_digest_idx_async")

    def digest_idx(self, state: AWSetBatch, idx, digest, tombs: TombBatch = None, mode: int = abi.CRDT_DIGEST_GATHER):
        """Host batch, host list and host digest array (numpy u64 [n_docs, 2]) uploaded, the
        listed docs re-digested on the device: the updated array, numpy u64 [n_docs, 2] (for
        tests and small callers)."""
        import numpy as np
        import torch

        dev = torch.device("cuda", self.device)
        state = state.numpy()
        digest = np.ascontiguousarray(digest, np.uint64).reshape(-1, 2)
        idx = np.ascontiguousarray(idx, np.uint32).reshape(-1)
        out = torch.zeros(max(2 * len(digest), 2), dtype=torch.int64, device=dev)
        out[: 2 * len(digest)] = torch.from_numpy(digest.reshape(-1).view(np.int64).copy()).to(dev)
        di = torch.zeros(max(len(idx), 1), dtype=torch.int32, device=dev)
        di[: len(idx)] = torch.from_numpy(idx.view(np.int32).copy()).to(dev)
        ds, dt = state.to(dev), tombs.numpy().to(dev) if tombs is not None else None
        s = ds.c()
        t = dt.c() if dt is not None else None
        check(self._lib.crdt_awset_digest_idx_async(self._ctx, ctypes.byref(s), ctypes.byref(t) if t else None,
                                                    ptr(di), None, len(idx), len(digest), int(mode), ptr(out), None),
              "crdt_awset_digest_idx_async")
        self.sync()
        return _np(out, np.uint64)[: 2 * len(digest)].reshape(len(digest), 2)

    def digest_diff_async(self, mine, theirs, n_docs: int, out: CompareBuffers, mask: int = 3, stream=None):
        """Per doc, CRDT_DIG_ELEMENTS / CRDT_DIG_STATE of two digest arrays (device u64
        [2 * n_docs]), the summary counts and the ascending worklist of docs with flags & mask,
        as compare_async writes them (crdt_digest_diff_async)."""
        co = _c(out)
        check(self._lib.crdt_digest_diff_async(self._ctx, ptr(mine), ptr(theirs), int(n_docs), int(mask),
                                               ctypes.byref(co), _stream(stream)), "crdt_digest_diff_async")

    def digest_tree_async(self, digest, n_docs: int, tree, stream=None):
        """The hash tree of fan-out 16 over a digest array (device u64 [2 * n_docs]) into
        `tree` (device u64, DigestTreeBuffers.tree), every level (crdt_digest_tree_async)."""
        check(self._lib.crdt_digest_tree_async(self._ctx, ptr(digest), int(n_docs), ptr(tree), _stream(stream)),
              "crdt_digest_tree_async")

    def digest_tree(self, digest):
        """Host digest array (numpy u64 [n_docs, 2]) uploaded and its tree built on the
        device: numpy u64 [n_nodes, 2] (for tests and small callers: digest_tree_host)."""
        import numpy as np
        import torch

        dev = torch.device("cuda", self.device)
        digest = np.ascontiguousarray(digest, np.uint64).reshape(-1, 2)
        bufs = DigestTreeBuffers(len(digest), dev)
        d = torch.zeros(max(2 * len(digest), 2), dtype=torch.int64, device=dev)
        d[: 2 * len(digest)] = torch.from_numpy(digest.reshape(-1).view(np.int64).copy()).to(dev)
        self.digest_tree_async(d, len(digest), bufs.tree)
        self.sync()
        return _np(bufs.tree, np.uint64)[: 2 * bufs.n_nodes].reshape(bufs.n_nodes, 2)

    def digest_tree_children_async(self, level, n_level: int, out, parents=None, n_parents=None, n_max=None,
                                   stream=None):
        """The sender's side of a descent: both words of the 16 children of every listed
        parent, packed into `out` (device u64, 32 words per parent), zeros past the level
        (crdt_digest_tree_children_async).  level: the node array the children lie in
        (DigestTreeBuffers.level).  parents / n_parents: device u32 list and count (a diff's
        idx_out / n_out); parents None: the identity, n_parents None: n_max."""
        n_max = int(parents.shape[0]) if n_max is None else int(n_max)
        check(self._lib.crdt_digest_tree_children_async(self._ctx, ptr(level), int(n_level), ptr(parents),
                                                        ptr(n_parents), n_max, ptr(out), _stream(stream)),
              "crdt_digest_tree_children_async")

    def digest_tree_diff_async(self, mine_level, n_level: int, theirs, idx_out, n_out, parents=None, n_parents=None,
                               n_max=None, leaf: bool = False, mask: int = 3, flags_out=None, out_max=None,
                               summary=None, stream=None):
        """The receiver's side: the listed parents' children of its own level against the
        peer's packed ones (`theirs`); the children with flag & mask ascending into idx_out,
        their flags into flags_out, their exact number into n_out (crdt_digest_tree_diff_async).
        leaf: the children are docs, flags as digest_diff_async; else nodes, bit 0 word 0
        differs, bit 1 word 1 differs.  idx_out / n_out are the next level's parents /
        n_parents.  out_max None: len(idx_out)."""
        n_max = int(parents.shape[0]) if n_max is None else int(n_max)
        out_max = int(idx_out.shape[0]) if out_max is None else int(out_max)
        check(self._lib.crdt_digest_tree_diff_async(self._ctx, ptr(mine_level), int(n_level), ptr(theirs),
                                                    ptr(parents), ptr(n_parents), n_max, 1 if leaf else 0, int(mask),
                                                    ptr(idx_out), ptr(flags_out), ptr(n_out), out_max, ptr(summary),
                                                    _stream(stream)), "crdt_digest_tree_diff_async")

    def digest_tree_descend(self, digest, tree: DigestTreeBuffers, fetch, mask: int = 3, start_level=None,
                            stream=None):
        """Drive a descent from level `start_level` (None: the root) down to the docs.
        fetch(level, parents, n) stands for the network: it returns the peer's packed
        children (device u64 [32 * n]) of the n nodes of `level` that the device list
        `parents` names (None: nodes 0 .. n - 1), as the peer's digest_tree_children_async
        writes them.  Between levels only the 4-byte n_out is read, to size the next
        request.  Returns (worklist, flags, n, bytes_fetched): device u32 doc ids ascending,
        their u8 flags (CRDT_DIG_*), their number, and 256 B per parent asked for.  The
        lists live in `tree` (built with cap >= the largest list of any level) and are
        overwritten by the next descent.  A list above cap raises CRDT_E_CAPACITY."""
        import numpy as np

        if tree.cap is None:
            raise ValueError("digest_tree_descend needs DigestTreeBuffers built with cap: the lists' room")
        if tree.L == 0:
            return tree.idx[0][:0], tree.flags[:0], 0, 0
        lvl = tree.L if start_level is None else int(start_level)
        if not 1 <= lvl <= tree.L:
            raise ValueError("start_level must be 1 .. L")
        parents, n = None, tree.nodes[lvl]
        if n > tree.cap:
            raise ValueError("start level holds more nodes than the buffers' cap")
        fetched, k = 0, 0
        while lvl >= 1:
            theirs = fetch(lvl, parents, n)
            fetched += 256 * n
            mine, n_level = tree.level(lvl - 1, digest)
            self.digest_tree_diff_async(mine, n_level, theirs, tree.idx[k], tree.n_out[k], parents=parents, n_max=n,
                                        leaf=lvl == 1, mask=mask, flags_out=tree.flags, out_max=tree.cap,
                                        summary=tree.summary, stream=stream)
            self.sync(stream)  # (also where a list above cap surfaces)
            n = int(_np(tree.n_out[k], np.uint32)[0])
            parents, k, lvl = tree.idx[k], k ^ 1, lvl - 1
            if n == 0:
                break
        return parents[:n], tree.flags[:n], n, fetched

    def select_async(self, state: AWSetBatch, out: OutBuffers, idx=None, n_idx=None, n_out=None, out_slots=None,
                     stream=None):
        """out doc j = state doc idx[j] (live entries, count, VV) for j < *n_idx, empty beyond,
        packed with no slack (crdt_awset_select_async).  idx / n_idx: device u32 arrays (a
        compare's worklist / n_work); None: the identity / n_out.  All None: compaction."""
        cs, co = _c(state), _c(out)
        n_out = out.n_docs if n_out is None else n_out
        out_slots = out.slots if out_slots is None else out_slots
        check(self._lib.crdt_awset_select_async(self._ctx, ctypes.byref(cs), ptr(idx), ptr(n_idx), int(n_out),
                                                int(out_slots), ctypes.byref(co), _stream(stream)),
              "crdt_awset_select_async")

    def scatter_async(self, state: AWSetBatch, sub: AWSetBatch, idx, out: OutBuffers, n_idx=None, out_slots=None,
                      stream=None):
        """out doc d = sub doc j when idx[j] == d for some j < *n_idx, else state doc d (live
        entries, count, VV), packed with no slack: select's inverse (crdt_awset_scatter_async).
        idx / n_idx: device u32 arrays (a compare's worklist / n_work); n_idx None: sub.n_docs.
        sub is typically the as_batch() of an exchange over the selected sub-batches."""
        cs, cb, co = _c(state), _c(sub), _c(out)
        out_slots = out.slots if out_slots is None else out_slots
        check(self._lib.crdt_awset_scatter_async(self._ctx, ctypes.byref(cs), ctypes.byref(cb), ptr(idx), ptr(n_idx),
                                                 int(out_slots), ctypes.byref(co), _stream(stream)),
              "crdt_awset_scatter_async")

    def sources_async(self, replicas, out: SrcBuffers, entry_slots=None, tomb_slots=None, stream=None):
        """Resident replicas (a list of Replica, in fold order) gathered into the packed
        source batch `out`: source d * P + p = replica p's doc d, live entries and
        tombstones only (crdt_awset_sources_async).  out is then a valid `srcs` of
        fold_async and delta_extract_async as it stands.  The slot limits default to the
        sizes of out's entry and tombstone arrays."""
        cr = [_c(r) for r in replicas]
        arr = (abi.CReplica * max(len(cr), 1))(*cr)
        o = out.c_delta_out()
        if entry_slots is None:
            entry_slots = int(out.keys.shape[0])
        if tomb_slots is None:
            tomb_slots = int(out.tkeys.shape[0]) if out.tkeys is not None else 0
        check(self._lib.crdt_awset_sources_async(self._ctx, arr, len(cr), int(entry_slots), int(tomb_slots),
                                                 ctypes.byref(o), _stream(stream)), "crdt_awset_sources_async")

    def sources(self, replicas) -> SrcBatch:
        """Host replicas uploaded, gathered on the device and the source batch downloaded,
        trimmed to its packed sizes (for tests and small callers: a caller who holds host
        data packs it on the host)."""
        import torch

        reps = [r.numpy() for r in replicas]
        n, R, P = reps[0].n_docs, reps[0].state.R, len(reps)
        ne = sum(r.state.live_slots() for r in reps)
        nt = sum(int(r.tombs.offsets[-1]) - int(r.tombs.offsets[0]) for r in reps if r.tombs is not None)
        dev = torch.device("cuda", self.device)
        out = SrcBuffers(R, n, n * P, ne, nt, device=dev)
        self.sources_async([r.to(dev) for r in reps], out, entry_slots=ne, tomb_slots=nt)
        self.sync()
        h = out.numpy()
        te, tt = int(h.entry_off[-1]), int(h.tomb_off[-1])
        return SrcBatch(R, h.doc_srcs, h.src_actor, h.vv[: n * P * R], h.entry_off, h.keys[:te], h.actors[:te],
                        h.counters[:te], h.tomb_off, h.tkeys[:tt], h.tactors[:tt], h.tcounters[:tt])

    def delta_join_async(self, dst: AWSetBatch, src, out: OutBuffers, kind=None, stream=None):
        """out[d] = dst[d] <- src[d] by (*AWSetDelta).Merge, src a resident Replica as it
        stands (crdt_awset_delta_join_async); kind: device u8 per doc, CRDT_DELTA_*, or None."""
        d, s, o = _c(dst), _c(src), _c(out)
        check(self._lib.crdt_awset_delta_join_async(self._ctx, ctypes.byref(d), ctypes.byref(s), ctypes.byref(o),
                                                    ptr(kind), _stream(stream)), "crdt_awset_delta_join_async")

    def delta_exchange_async(self, a, b, out_ab: OutBuffers, out_ba: OutBuffers, kind_ab=None, kind_ba=None,
                             stream=None):
        """Both AWSetDelta merges of a resident Replica pair from one read of both:
        out_ab = a <- b and out_ba = b <- a, in the join's layout
        (crdt_awset_delta_exchange_async); kind_ab / kind_ba: device u8 per doc, or None."""
        ca, cb, o1, o2 = _c(a), _c(b), _c(out_ab), _c(out_ba)
        check(self._lib.crdt_awset_delta_exchange_async(self._ctx, ctypes.byref(ca), ctypes.byref(cb),
                                                        ctypes.byref(o1), ctypes.byref(o2), ptr(kind_ab),
                                                        ptr(kind_ba), _stream(stream)),
              "crdt_awset_delta_exchange_async")

    def delta_exchange(self, a, b):
        """Host replicas uploaded, exchanged on the device and downloaded: (out_ab, out_ba,
        kind_ab, kind_ba), the outputs as host OutBuffers and the kinds as numpy uint8 arrays
        (for tests and small callers: a caller who holds host data builds a source batch and folds)."""
        import numpy as np
        import torch

        a, b = a.numpy(), b.numpy()
        n, R = a.n_docs, a.state.R
        slots = int(a.state.offsets[-1]) + int(b.state.offsets[-1])
        dev = torch.device("cuda", self.device)
        outs = [OutBuffers(n, R, slots, device=dev) for _ in range(2)]
        kinds = [torch.zeros(max(n, 1), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.delta_exchange_async(a.to(dev), b.to(dev), outs[0], outs[1], kinds[0], kinds[1])
        self.sync()
        host = []
        for o in outs:
            h = OutBuffers(n, R, slots)
            h.offsets, h.counts, h.vv = _np(o.offsets, np.uint32), _np(o.counts, np.uint32), _np(o.vv, np.uint64)
            h.keys, h.actors, h.counters = _np(o.keys, np.uint64), _np(o.actors, np.uint32), _np(o.counters, np.uint64)
            host.append(h)
        return host[0], host[1], _np(kinds[0], np.uint8)[:n], _np(kinds[1], np.uint8)[:n]

    def delta_join_log_async(self, dst: AWSetBatch, src, out: OutBuffers, log: MergeLogBuffers, kind=None,
                             stream=None):
        """delta_join_async with the merge's log written beside the merged state: per doc, the
        dst entries removed (in dst's slot layout) and the src entries added or moved to (in
        src's), with CRDT_DIFF_* flags and the summary -- what diff_async(dst, out) reports,
        from the one read the merge needs (crdt_awset_delta_join_log_async)."""
        d, s, o, lg = _c(dst), _c(src), _c(out), _c(log)
        check(self._lib.crdt_awset_delta_join_log_async(self._ctx, ctypes.byref(d), ctypes.byref(s), ctypes.byref(o),
                                                        ptr(kind), ctypes.byref(lg), _stream(stream)),
              "crdt_awset_delta_join_log_async")

    def delta_exchange_log_async(self, a, b, out_ab: OutBuffers, out_ba: OutBuffers, log_ab: MergeLogBuffers,
                                 log_ba: MergeLogBuffers, kind_ab=None, kind_ba=None, stream=None):
        """delta_exchange_async with both directions' logs, from one read of both replicas:
        log_ab removed in a's layout and upserted in b's, log_ba the other way round
        (crdt_awset_delta_exchange_log_async)."""
        ca, cb, o1, o2, l1, l2 = _c(a), _c(b), _c(out_ab), _c(out_ba), _c(log_ab), _c(log_ba)
        check(self._lib.crdt_awset_delta_exchange_log_async(self._ctx, ctypes.byref(ca), ctypes.byref(cb),
                                                            ctypes.byref(o1), ctypes.byref(o2), ptr(kind_ab),
                                                            ptr(kind_ba), ctypes.byref(l1), ctypes.byref(l2),
                                                            _stream(stream)),
              "crdt_awset_delta_exchange_log_async")

    def delta_exchange_log(self, a, b):
        """Host replicas uploaded, exchanged with the logs on the device and downloaded:
        (out_ab, out_ba, kind_ab, kind_ba, log_ab, log_ba), the outputs as host OutBuffers, the
        kinds as numpy uint8 arrays and the logs as MergeLogBuffers.numpy() (for tests and
        small callers)."""
        import numpy as np
        import torch

        a, b = a.numpy(), b.numpy()
        n, R = a.n_docs, a.state.R
        sa, sb = int(a.state.offsets[-1]), int(b.state.offsets[-1])
        dev = torch.device("cuda", self.device)
        outs = [OutBuffers(n, R, sa + sb, device=dev) for _ in range(2)]
        kinds = [torch.zeros(max(n, 1), dtype=torch.uint8, device=dev) for _ in range(2)]
        logs = [MergeLogBuffers(n, sa, sb, device=dev), MergeLogBuffers(n, sb, sa, device=dev)]
        self.delta_exchange_log_async(a.to(dev), b.to(dev), outs[0], outs[1], logs[0], logs[1], kinds[0], kinds[1])
        self.sync()
        host = []
        for o in outs:
            h = OutBuffers(n, R, sa + sb)
            h.offsets, h.counts, h.vv = _np(o.offsets, np.uint32), _np(o.counts, np.uint32), _np(o.vv, np.uint64)
            h.keys, h.actors, h.counters = _np(o.keys, np.uint64), _np(o.actors, np.uint32), _np(o.counters, np.uint64)
            host.append(h)
        return (host[0], host[1], _np(kinds[0], np.uint8)[:n], _np(kinds[1], np.uint8)[:n], logs[0].numpy(),
                logs[1].numpy())

    def replica_select_async(self, rep, out: ReplicaBuffers, idx=None, n_idx=None, n_out=None, entry_slots=None,
                             tomb_slots=None, stream=None):
        """select_async over a whole resident Replica: out doc j = rep doc idx[j] for
        j < *n_idx (live entries, count, VV, live tombstones, actor), empty beyond, entries
        and tombstones each packed with no slack (crdt_replica_select_async).  idx / n_idx:
        device u32 arrays (a worklist / n_work); all None: compaction of the replica.  The
        slot limits default to the sizes out was made with."""
        cr, co = _c(rep), _c(out)
        n_out = out.n_docs if n_out is None else n_out
        entry_slots = out.entry_slots if entry_slots is None else entry_slots
        tomb_slots = out.tomb_slots if tomb_slots is None else tomb_slots
        check(self._lib.crdt_replica_select_async(self._ctx, ctypes.byref(cr), ptr(idx), ptr(n_idx), int(n_out),
                                                  int(entry_slots), int(tomb_slots), ctypes.byref(co),
                                                  _stream(stream)), "crdt_replica_select_async")

    def replica_scatter_async(self, rep, sub, idx, out: ReplicaBuffers, n_idx=None, entry_slots=None,
                              tomb_slots=None, stream=None):
        """scatter_async over whole resident Replicas: out doc d = sub doc j when
        idx[j] == d for some j < *n_idx, else rep doc d, with its tombstones and actor
        (crdt_replica_scatter_async).  sub is typically a delta exchange's or an apply's
        output over the selected sub-replica, with the selected tombstones and actors."""
        cr, cs, co = _c(rep), _c(sub), _c(out)
        entry_slots = out.entry_slots if entry_slots is None else entry_slots
        tomb_slots = out.tomb_slots if tomb_slots is None else tomb_slots
        check(self._lib.crdt_replica_scatter_async(self._ctx, ctypes.byref(cr), ctypes.byref(cs), ptr(idx),
                                                   ptr(n_idx), int(entry_slots), int(tomb_slots), ctypes.byref(co),
                                                   _stream(stream)), "crdt_replica_scatter_async")

    @staticmethod
    def _tomb_live(rep) -> int:
        if rep.tombs is None:
            return 0
        if rep.tombs.counts is not None:
            return int(rep.tombs.counts.astype("uint64").sum())
        return int(rep.tombs.offsets[-1]) - int(rep.tombs.offsets[0])

    def replica_select(self, rep, idx=None, n_idx=None, n_out=None):
        """Host Replica uploaded, selected on the device and downloaded as a Replica trimmed
        to its packed sizes (for tests and small callers).  idx: host u32 array or None;
        n_idx: int or None."""
        import numpy as np
        import torch

        rep = rep.numpy()
        dev = torch.device("cuda", self.device)
        n_out = (rep.n_docs if idx is None else len(idx)) if n_out is None else int(n_out)
        reps = max(1, -(-n_out // max(rep.n_docs, 1)))  # an idx that repeats may select a document many times
        out = ReplicaBuffers(n_out, rep.state.R, rep.state.live_slots() * reps, self._tomb_live(rep) * reps,
                             device=dev, tombs=rep.tombs is not None)
        didx = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, np.uint32).view(np.int32)).to(dev)
        dn = None if n_idx is None else torch.tensor([int(n_idx)], dtype=torch.int32, device=dev)
        self.replica_select_async(rep.to(dev), out, didx, dn)
        self.sync()
        return out.numpy()

    def replica_scatter(self, rep, sub, idx, n_idx=None):
        """Host Replicas uploaded, scattered on the device and downloaded as a Replica
        trimmed to its packed sizes (for tests and small callers)."""
        import numpy as np
        import torch

        rep, sub = rep.numpy(), sub.numpy()
        dev = torch.device("cuda", self.device)
        out = ReplicaBuffers(rep.n_docs, rep.state.R, rep.state.live_slots() + sub.state.live_slots(),
                             self._tomb_live(rep) + self._tomb_live(sub), device=dev,
                             tombs=rep.tombs is not None or sub.tombs is not None)
        didx = torch.from_numpy(np.ascontiguousarray(idx, np.uint32).view(np.int32)).to(dev)
        if didx.numel() == 0:
            didx = torch.zeros(1, dtype=torch.int32, device=dev)
        dn = None if n_idx is None else torch.tensor([int(n_idx)], dtype=torch.int32, device=dev)
        self.replica_scatter_async(rep.to(dev), sub.to(dev), didx, out, dn)
        self.sync()
        return out.numpy()

    def replica_scatter_inplace_async(self, target, sub, idx, spill: SpillBuffers, n_idx=None, stream=None):
        """replica_scatter_async without the packed copy: sub doc j is written into the
        slots `target` doc idx[j] already owns when its live entries and tombstones fit
        them (count, clock, tombstone count and actor with it), and is listed in `spill`
        otherwise; nothing else of target is touched (crdt_replica_scatter_inplace_async).
        target: an InplaceTarget, or what InplaceTarget.of() views as one (a Replica with
        counts, a ReplicaBuffers); sub: a Replica."""
        ct = target if isinstance(target, ctypes.Structure) else _c(InplaceTarget.of(target))
        cs, cp = _c(sub), _c(spill)
        check(self._lib.crdt_replica_scatter_inplace_async(self._ctx, ctypes.byref(ct), ctypes.byref(cs), ptr(idx),
                                                           ptr(n_idx), ctypes.byref(cp), _stream(stream)),
              "crdt_replica_scatter_inplace_async")

    def scatter_inplace_async(self, state, sub: AWSetBatch, idx, spill: SpillBuffers, n_idx=None, stream=None):
        """replica_scatter_inplace_async for state-only batches: `state` (an AWSetBatch
        with counts, or an OutBuffers) receives sub's documents in place; no tombstones,
        no actors."""
        tgt = InplaceTarget.of(state, actors=False)
        self.replica_scatter_inplace_async(InplaceTarget(tgt.state), Replica(sub), idx, spill, n_idx, stream)

    def replica_scatter_inplace(self, rep, sub, idx, n_idx=None):
        """Host Replicas uploaded, sub scattered into rep in place on the device, and
        downloaded: (rep as it then stands, same layout; spill_j; spill_doc)."""
        import numpy as np
        import torch

        rep, sub = rep.numpy(), sub.numpy()
        dev = torch.device("cuda", self.device)
        if rep.state.counts is None:
            o = rep.state.offsets
            rep.state.counts = (o[1:] - o[:-1]).astype(np.uint32)
        if rep.tombs is not None and rep.tombs.counts is None:
            o = rep.tombs.offsets
            rep.tombs.counts = (o[1:] - o[:-1]).astype(np.uint32)
        drep = rep.to(dev)
        spill = SpillBuffers(sub.n_docs, device=dev)
        didx = torch.from_numpy(np.ascontiguousarray(idx, np.uint32).view(np.int32)).to(dev)
        if didx.numel() == 0:
            didx = torch.zeros(1, dtype=torch.int32, device=dev)
        dn = None if n_idx is None else torch.tensor([int(n_idx)], dtype=torch.int32, device=dev)
        self.replica_scatter_inplace_async(drep, sub.to(dev), didx, spill, dn)
        self.sync()
        sj, sd = spill.numpy()
        return drep.numpy(), sj, sd

    def replica_repack_async(self, rep, out: ReplicaBuffers, sub=None, idx=None, n_idx=None, n_out=None,
                             entry_room: Headroom = None, tomb_room: Headroom = None, entry_slots=None,
                             tomb_slots=None, stream=None):
        """replica_select_async (sub None) or replica_scatter_async (sub a Replica, idx its
        documents' places) writing a layout with headroom: out doc j owns
        entry_room.capacity(live entries) entry slots and tomb_room.capacity(live
        tombstones) tombstone slots, offsets their prefix, counts the live counts, and
        nothing at or past a live count is written (crdt_replica_repack_async).  A room
        of None is packed.  out is a Replica (out.as_replica()) and an in-place target
        (InplaceTarget.of(out)) as it stands."""
        cr, co = _c(rep), _c(out)
        cs = _c(sub) if sub is not None else None
        n_out = (out.n_docs if sub is None else rep.n_docs) if n_out is None else n_out
        entry_slots = out.entry_slots if entry_slots is None else entry_slots
        tomb_slots = out.tomb_slots if tomb_slots is None else tomb_slots
        er = entry_room.c() if entry_room is not None else None
        tr = tomb_room.c() if tomb_room is not None else None
        check(self._lib.crdt_replica_repack_async(self._ctx, ctypes.byref(cr), ctypes.byref(cs) if cs is not None else None,
                                                  ptr(idx), ptr(n_idx), int(n_out),
                                                  ctypes.byref(er) if er is not None else None,
                                                  ctypes.byref(tr) if tr is not None else None, int(entry_slots),
                                                  int(tomb_slots), ctypes.byref(co), _stream(stream)),
              "crdt_replica_repack_async")

    def replica_repack(self, rep, sub=None, idx=None, n_idx=None, n_out=None, entry_room=None, tomb_room=None):
        """Host Replicas uploaded, repacked on the device and downloaded: (Replica, code).
        The Replica keeps its layout (offsets the prefix of the capacities, columns as
        long as the capacity totals, slack zeroed by the allocation), so
        InplaceTarget.of() takes it as it stands; code is what crdt_ctx_sync reports
        (0: CRDT_OK).  The buffers are sized from a first call with no slots, which
        writes the live counts."""
        import numpy as np
        import torch

        rep = rep.numpy()
        sub = sub.numpy() if sub is not None else None
        dev = torch.device("cuda", self.device)
        if sub is not None:
            n_out = rep.n_docs
        else:
            n_out = (rep.n_docs if idx is None else len(idx)) if n_out is None else int(n_out)
        tombs = rep.tombs is not None or (sub is not None and sub.tombs is not None)
        didx = None if idx is None else torch.from_numpy(np.ascontiguousarray(idx, np.uint32).view(np.int32)).to(dev)
        if didx is not None and didx.numel() == 0:
            didx = torch.zeros(1, dtype=torch.int32, device=dev)
        dn = None if n_idx is None else torch.tensor([int(n_idx)], dtype=torch.int32, device=dev)
        drep, dsub = rep.to(dev), sub.to(dev) if sub is not None else None
        kw = dict(sub=dsub, idx=didx, n_idx=dn, n_out=n_out, entry_room=entry_room, tomb_room=tomb_room)
        probe = ReplicaBuffers(n_out, rep.state.R, 0, 0, device=dev, tombs=tombs)
        self.replica_repack_async(drep, probe, **kw)
        self._lib.crdt_ctx_sync(self._ctx, None)  # (CRDT_E_CAPACITY by construction: nothing fits no slots)
        es = (entry_room or Headroom()).total(_np(probe.state.counts, np.uint32)[:n_out])
        ts = (tomb_room or Headroom()).total(_np(probe.tombs.counts, np.uint32)[:n_out]) if tombs else 0
        out = ReplicaBuffers(n_out, rep.state.R, min(es, 0xFFFFFFFF), min(ts, 0xFFFFFFFF), device=dev, tombs=tombs)
        for b in (out.state, out.tombs):
            if b is not None:
                for f in ("keys", "actors", "counters"):
                    getattr(b, f).zero_()
        self.replica_repack_async(drep, out, **kw)
        code = int(self._lib.crdt_ctx_sync(self._ctx, None))
        return out.numpy(), code

    def vv_min_async(self, dst, src, n: int, stream=None):
        check(self._lib.crdt_vv_min_async(self._ctx, ptr(dst), ptr(src), int(n), _stream(stream)),
              "crdt_vv_min_async")

    # -- multi-GPU: global causal context over RCCL ------------------------
    def comm_init(self, n_ranks: int, rank: int, uid: bytes):
        """One process per GPU: join the communicator of `uid` (crdt_comm_unique_id on rank 0)."""
        buf = ctypes.create_string_buffer(bytes(uid), len(uid))
        check(self._lib.crdt_comm_init(self._ctx, int(n_ranks), int(rank), buf), "crdt_comm_init")

    def context_allreduce_async(self, vv_R, R: int, stream=None):
        """In-place u64 max of this rank's R-vector with every other rank's (RCCL)."""
        check(self._lib.crdt_context_allreduce_async(self._ctx, ptr(vv_R), int(R), _stream(stream)),
              "crdt_context_allreduce_async")

    def gen_pair_async(self, seed: int, n_docs: int, a: OutBuffers, b: OutBuffers, stream=None):
        ca, cb = a.c(), b.c()
        check(self._lib.crdt_gen_pair_async(self._ctx, int(seed), int(n_docs), ctypes.byref(ca), ctypes.byref(cb),
                                            _stream(stream)), "crdt_gen_pair_async")

    def gen_delta_async(self, seed: int, n_docs: int, R: int, M: int, dst: OutBuffers, srcs: SrcBatch, stream=None):
        cd, cs = dst.c(), srcs.c()
        check(self._lib.crdt_gen_delta_async(self._ctx, int(seed), int(n_docs), int(R), int(M), ctypes.byref(cd),
                                             ctypes.byref(cs), _stream(stream)), "crdt_gen_delta_async")

    def gen_replicas_async(self, seed: int, n_docs: int, P: int, E: int, dst: OutBuffers, srcs: SrcBatch,
                           stream=None):
        cd, cs = dst.c(), srcs.c()
        check(self._lib.crdt_gen_replicas_async(self._ctx, int(seed), int(n_docs), int(P), int(E), ctypes.byref(cd),
                                                ctypes.byref(cs), _stream(stream)), "crdt_gen_replicas_async")

    def gen_zipf_async(self, seed: int, n_docs: int, offsets, a: OutBuffers, b: OutBuffers, stream=None):
        ca, cb = a.c(), b.c()
        check(self._lib.crdt_gen_zipf_async(self._ctx, int(seed), int(n_docs), ptr(offsets), ctypes.byref(ca),
                                            ctypes.byref(cb), _stream(stream)), "crdt_gen_zipf_async")

    # -- host buffers, synchronous ----------------------------------------
    def join(self, dst: AWSetBatch, src: AWSetBatch, pinned: bool = False) -> OutBuffers:
        """Host buffers; pinned: the output in page-locked memory (crdt_host_alloc)."""
        dst, src = dst.numpy(), src.numpy()
        out = OutBuffers(dst.n_docs, dst.R, int(dst.offsets[-1]) + int(src.offsets[-1]), pinned=pinned)
        d, s, o = dst.c(), src.c(), out.c()
        check(self._lib.crdt_awset_join_batch(self._ctx, ctypes.byref(d), ctypes.byref(s), ctypes.byref(o)),
              "crdt_awset_join_batch")
        return out

    def exchange(self, a: AWSetBatch, b: AWSetBatch, shared_keys: bool = False, pinned: bool = False):
        """Host buffers: (a <- b, b <- a); shared_keys: both outputs use one key column;
        pinned: the outputs in page-locked memory (crdt_host_alloc)."""
        a, b = a.numpy(), b.numpy()
        slots = int(a.offsets[-1]) + int(b.offsets[-1])
        o1 = OutBuffers(a.n_docs, a.R, slots, pinned=pinned)
        o2 = OutBuffers(a.n_docs, a.R, slots, shared_keys=o1 if shared_keys else None, pinned=pinned)
        ca, cb, c1, c2 = a.c(), b.c(), o1.c(), o2.c()
        check(self._lib.crdt_awset_exchange_batch(self._ctx, ctypes.byref(ca), ctypes.byref(cb), ctypes.byref(c1),
                                                  ctypes.byref(c2)), "crdt_awset_exchange_batch")
        return o1, o2

    def apply(self, state: AWSetBatch, ops: OpBatch, tombs: TombBatch = None, with_tombs: bool = True):
        """Host buffers: (entries out, tombstones out or None) after each doc's ops."""
        state, ops = state.numpy(), ops.numpy()
        tombs = tombs.numpy() if tombs is not None else None
        nops = int(ops.op_off[-1])
        out = OutBuffers(state.n_docs, state.R, int(state.offsets[-1]) + nops)
        tout = TombBuffers(state.n_docs, (int(tombs.offsets[-1]) if tombs is not None else 0) + nops) \
            if with_tombs else None
        cs, co, cout = state.c(), ops.c(), out.c()
        ct = tombs.c() if tombs is not None else None
        cto = tout.c_out() if tout is not None else None
        check(self._lib.crdt_awset_apply_batch(self._ctx, ctypes.byref(cs), ctypes.byref(ct) if ct else None,
                                               ctypes.byref(co), ctypes.byref(cout),
                                               ctypes.byref(cto) if cto else None), "crdt_awset_apply_batch")
        return out, tout

    def delta_extract(self, srcs: SrcBatch, peer_vv):
        """Host buffers: (the message as a SrcBatch trimmed to its packed sizes,
        kind per source as a numpy uint8 array)."""
        import numpy as np

        srcs = srcs.numpy()
        ns = int(srcs.doc_srcs[-1])
        ne = int(srcs.entry_off[ns])
        nt = int(srcs.tomb_off[ns]) if srcs.tomb_off is not None else 0
        peer = _np(peer_vv if hasattr(peer_vv, "dtype") else np.asarray(peer_vv, dtype=np.uint64), np.uint64)
        out = SrcBuffers(srcs.R, srcs.n_docs, ns, ne, nt)
        kind = np.zeros(max(ns, 1), dtype=np.uint8)
        s, o = srcs.c(), out.c_delta_out(kind)
        check(self._lib.crdt_awset_delta_extract_batch(self._ctx, ctypes.byref(s), ptr(peer), ctypes.byref(o)),
              "crdt_awset_delta_extract_batch")
        te, tt = int(out.entry_off[ns]), int(out.tomb_off[ns])
        msg = SrcBatch(srcs.R, out.doc_srcs, out.src_actor, out.vv[: ns * srcs.R], out.entry_off, out.keys[:te],
                       out.actors[:te], out.counters[:te], out.tomb_off, out.tkeys[:tt], out.tactors[:tt],
                       out.tcounters[:tt])
        return msg, kind[:ns]

    def has(self, state: AWSetBatch, queries: QueryBatch):
        """Host buffers: (found, actors, counters) numpy arrays, one per query
        (crdt_awset_has_batch; for tests and small callers)."""
        state, queries = state.numpy(), queries.numpy()
        out = QueryBuffers(queries.n_queries)
        s, q, o = state.c(), queries.c(), out.c()
        check(self._lib.crdt_awset_has_batch(self._ctx, ctypes.byref(s), ctypes.byref(q), ctypes.byref(o)),
              "crdt_awset_has_batch")
        return out.numpy()

    def compare(self, a: AWSetBatch, b: AWSetBatch, mask: int = 15):
        """Host buffers: (flags, summary, worklist) numpy arrays (crdt_awset_compare_batch;
        for tests and small callers)."""
        a, b = a.numpy(), b.numpy()
        out = CompareBuffers(a.n_docs)
        ca, cb, co = a.c(), b.c(), out.c()
        check(self._lib.crdt_awset_compare_batch(self._ctx, ctypes.byref(ca), ctypes.byref(cb), int(mask),
                                                 ctypes.byref(co)), "crdt_awset_compare_batch")
        return out.numpy()

    def diff(self, before: AWSetBatch, after: AWSetBatch):
        """Host buffers: DiffBuffers.numpy() of the diff, its lists sized from the totals
        (crdt_awset_diff_batch; for tests and small callers).  One call with a worst-case
        allocation, not a sizing call and an emitting call: a removed record is a live entry
        of `before` and an upsert a live entry of `after`, so the live counts bound the
        totals, and only the first `total` words of each list are downloaded."""
        before, after = before.numpy(), after.numpy()
        out = DiffBuffers(before.n_docs, before.live_slots(), after.live_slots())
        cb, ca, co = before.c(), after.c(), out.c()
        check(self._lib.crdt_awset_diff_batch(self._ctx, ctypes.byref(cb), ctypes.byref(ca), out.rem_slots,
                                              out.ups_slots, ctypes.byref(co)), "crdt_awset_diff_batch")
        return out.numpy()

    def fold(self, mode: int, dst: AWSetBatch, srcs: SrcBatch, pinned: bool = False) -> OutBuffers:
        dst, srcs = dst.numpy(), srcs.numpy()
        out = OutBuffers(dst.n_docs, dst.R, srcs.out_slots(dst), pinned=pinned)
        d, s, o = dst.c(), srcs.c(), out.c()
        check(self._lib.crdt_awset_fold_batch(self._ctx, int(mode), ctypes.byref(d), ctypes.byref(s),
                                              ctypes.byref(o)), "crdt_awset_fold_batch")
        return out


def comm_unique_id() -> bytes:
    """A fresh RCCL communicator id (rank 0 makes it, every rank passes it to comm_init)."""
    buf = ctypes.create_string_buffer(128)
    check(abi.lib().crdt_comm_unique_id(buf), "crdt_comm_unique_id")
    return buf.raw


def global_context_allreduce(engines, vvs, R: int):
    """One process, one Engine per GPU: every vvs[i] (device R-vector on engine i's
    GPU) becomes the elementwise u64 max over all of them; returns it as a list."""
    n = len(engines)
    ctxs = (ctypes.c_void_p * n)(*[e._ctx for e in engines])
    ptrs = (ctypes.c_void_p * n)(*[ptr(v) for v in vvs])
    out = (ctypes.c_uint64 * int(R))()
    check(abi.lib().crdt_global_context_allreduce(ctxs, n, ptrs, int(R), ctypes.cast(out, ctypes.c_void_p)),
          "crdt_global_context_allreduce")
    return [int(x) for x in out]


def format_doc(batch: AWSetBatch, d: int, names=None) -> str:
    """Go's (AWSet).String() of doc d of a host batch (crdt_awset_format); names[id] = key string."""
    b = batch.numpy()
    cb = b.c()
    arr = None
    if names is not None:
        enc = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
        arr = (ctypes.c_char_p * len(enc))(*enc)
    n = ctypes.c_size_t(0)
    check(abi.lib().crdt_awset_format(ctypes.byref(cb), int(d), arr, None, 0, ctypes.byref(n)), "crdt_awset_format")
    buf = ctypes.create_string_buffer(n.value + 1)
    check(abi.lib().crdt_awset_format(ctypes.byref(cb), int(d), arr, buf, n.value + 1, ctypes.byref(n)),
          "crdt_awset_format")
    return buf.raw[: n.value].decode("utf-8", errors="surrogateescape")


def dump_batch(batch: AWSetBatch) -> bytes:
    """Self-checking binary image of a host batch (crdt_batch_dump)."""
    b = batch.numpy()
    cb = b.c()
    n = ctypes.c_size_t(0)
    check(abi.lib().crdt_batch_dump(ctypes.byref(cb), None, 0, ctypes.byref(n)), "crdt_batch_dump")
    buf = ctypes.create_string_buffer(n.value)
    check(abi.lib().crdt_batch_dump(ctypes.byref(cb), buf, n.value, ctypes.byref(n)), "crdt_batch_dump")
    return buf.raw


def load_batch(image: bytes) -> AWSetBatch:
    """Inverse of dump_batch: a compact host batch (crdt_batch_info + crdt_batch_undump)."""
    import numpy as np

    nd, R, ne = ctypes.c_uint32(0), ctypes.c_uint32(0), ctypes.c_uint64(0)
    buf = ctypes.create_string_buffer(bytes(image), len(image))
    check(abi.lib().crdt_batch_info(buf, len(image), ctypes.byref(nd), ctypes.byref(R), ctypes.byref(ne)),
          "crdt_batch_info")
    out = OutBuffers(nd.value, R.value, ne.value)
    co = out.c()
    check(abi.lib().crdt_batch_undump(buf, len(image), ctypes.byref(co)), "crdt_batch_undump")
    return AWSetBatch(R.value, out.offsets, out.keys, out.actors, out.counters, out.vv,
                      counts=out.counts if nd.value else np.zeros(0, np.uint32))


def zipf_sizes(seed: int, n_docs: int):
    """Document sizes of the "zipf" workload (host computation, no GPU)."""
    import numpy as np

    out = np.zeros(max(n_docs, 1), dtype=np.uint32)
    check(abi.lib().crdt_gen_zipf_sizes(int(seed), int(n_docs), out.ctypes.data), "crdt_gen_zipf_sizes")
    return out[:n_docs]


def digest_host(batch: AWSetBatch, tombs: TombBatch = None):
    """Per-doc digests of a host batch, numpy u64 [n_docs, 2] (crdt_awset_digest_host: no
    GPU; a doc's entries may lie in any order).  Raises CrdtError on a bad layout."""
    import numpy as np

    b = batch.numpy()
    cb = b.c()
    t = tombs.numpy() if tombs is not None else None
    ct = t.c() if t is not None else None
    out = np.zeros(max(2 * b.n_docs, 1), dtype=np.uint64)
    check(abi.lib().crdt_awset_digest_host(ctypes.byref(cb), ctypes.byref(ct) if ct else None, out.ctypes.data),
          "crdt_awset_digest_host")
    return out[: 2 * b.n_docs].reshape(b.n_docs, 2)


def digest_tree_layout(n_docs: int):
    """(L, nodes, off) of the digest tree over n_docs docs: nodes[l] the nodes of level l
    (nodes[0] = n_docs), off[l] the node offset of level l >= 1 in the tree array
    (crdt_digest_tree_layout)."""
    import numpy as np

    nodes, off = np.zeros(9, np.uint32), np.zeros(9, np.uint32)
    L = abi.lib().crdt_digest_tree_layout(int(n_docs), nodes.ctypes.data, off.ctypes.data)
    return int(L), [int(x) for x in nodes], [int(x) for x in off]


def digest_tree_host(digest):
    """The digest tree of a host digest array (numpy u64 [n_docs, 2]), numpy u64
    [n_nodes, 2], levels 1 .. L concatenated (crdt_digest_tree_host: no GPU)."""
    import numpy as np

    digest = np.ascontiguousarray(digest, np.uint64).reshape(-1, 2)
    L, nodes, off = digest_tree_layout(len(digest))
    n_nodes = off[L] + 1 if L else 0
    out = np.zeros(max(2 * n_nodes, 1), dtype=np.uint64)
    check(abi.lib().crdt_digest_tree_host(digest.ctypes.data, len(digest), out.ctypes.data), "crdt_digest_tree_host")
    return out[: 2 * n_nodes].reshape(n_nodes, 2)


def validate(batch: AWSetBatch) -> int:
    b = batch.numpy().c()
    return abi.lib().crdt_validate_batch(ctypes.byref(b))


def validate_src(srcs: SrcBatch) -> int:
    s = srcs.numpy().c()
    return abi.lib().crdt_validate_src_batch(ctypes.byref(s))


def validate_tombs(tombs, n_docs: int) -> int:
    t = tombs.numpy().c()
    return abi.lib().crdt_validate_tomb_batch(ctypes.byref(t), n_docs)
