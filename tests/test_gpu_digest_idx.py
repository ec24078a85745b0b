"""GPU: crdt_awset_digest_idx_async (csrc/digest_idx.hip) against
crdt_awset_digest_host of the whole replica, bit-exact, in both modes.

Every case of tests/digest_idx_cases.py runs into a digest array pre-filled with
a per-word sentinel (tests/test_digest_idx_model.py): the listed documents must
equal digest_host (host code, independent of the kernels) and
crdt_awset_digest_async of the same replica, every other word must still be its
sentinel.  Then the error table, run-to-run identity, graph capture with a
replay after the state and *n_idx changed, and the round the call exists for: a
replica with headroom, local ops on a 5 % selection, the in-place scatter, and
the digest array brought up to date by the worklist alone.
"""

import ctypes

import numpy as np
import pytest

import crdtgpu
from crdtgpu import CRDT_DIGEST_GATHER as GATHER
from crdtgpu import CRDT_DIGEST_PLACE as PLACE
from crdtgpu import CRDT_E_CAPACITY, CRDT_E_INVALID, abi
from crdtgpu.batch import AWSetBatch, OutBuffers, Replica, ReplicaBuffers, SpillBuffers, TombBatch, TombBuffers, _np
from digest_idx_cases import MAIN_NAMES, case, cases, listed, place_sub
from replica_repack_cases import ROUND_ROOM
from test_digest_idx_model import expected, full_digest, sentinel
from test_gpu_compare import _code, dev_of
from test_gpu_replica import shifted, word, words
from test_replica_inplace_model import replica_scatter_inplace_ref
from test_replica_model import apply_round_case, replica_select_ref
from test_replica_repack_model import replica_repack_ref

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64


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

def upload(torch, st, tb, shift=False):
    """(state, tombs) on the device; shift: every entry array one element past an aligned address."""
    dev = dev_of(torch)
    ds, dt = st.to(dev), tb.to(dev) if tb is not None else None
    if shift:
        ds = AWSetBatch(ds.R, ds.offsets, shifted(torch, ds.keys), shifted(torch, ds.actors),
                        shifted(torch, ds.counters), ds.vv, counts=ds.counts)
        if dt is not None:
            dt = TombBatch(dt.offsets, shifted(torch, dt.keys), shifted(torch, dt.actors), shifted(torch, dt.counters),
                           dt.counts)
        assert ds.keys.data_ptr() % 16 == 8 and ds.actors.data_ptr() % 8 == 4
    return ds, dt


def device_digest(torch, host, shift=False):
    t = torch.from_numpy(np.ascontiguousarray(host, U64).reshape(-1).view(np.int64).copy()).to(dev_of(torch))
    if t.numel() == 0:
        t = torch.zeros(2, dtype=torch.int64, device=dev_of(torch))
    return shifted(torch, t) if shift else t


def read_digest(t, n_docs):
    return _np(t, U64)[: 2 * n_docs].reshape(n_docs, 2)


def assert_digest(got, want, rows=None):
    assert got.shape == want.shape, (got.shape, want.shape)
    if not (got == want).all():
        d, w = [int(x[0]) for x in np.nonzero(got != want)]
        raise AssertionError("document %d word %d: gpu %#x, expected %#x (%d documents differ%s)"
                             % (d, w, int(got[d, w]), int(want[d, w]), int((got != want).any(axis=1).sum()),
                                ", listed" if rows is not None and d in rows else ""))


_dev = {}


def on_device(torch, c, mode):
    """(state, tombs) the call reads for the case in that mode, uploaded once."""
    key = (c.name, mode)
    if key not in _dev:
        st, tb = (c.state, c.tombs) if mode == GATHER else place_sub(c)
        _dev[key] = upload(torch, st, tb, c.shift)
    return _dev[key]


def run(eng, torch, c, mode, stream=None, engine=None):
    """The sentinel array after one call of the case (synced)."""
    ds, dt = on_device(torch, c, mode)
    n = c.state.n_docs
    dig = device_digest(torch, sentinel(n), shift=c.shift)  # (shifted: 8 B aligned only, the two-store form)
    e = engine or eng
    e.digest_idx_async(ds, words(torch, c.idx), dig, tombs=dt, n_idx=word(torch, c.n_idx), n_max=c.n_max, mode=mode,
                       stream=stream)
    e.sync(stream)
    return read_digest(dig, n)


# ------------------------------------------------------------------- 1. the case table

@pytest.mark.parametrize("name,mode", [(c.name, m) for c in cases() for m in (GATHER, PLACE)
                                       if not (m == PLACE and c.gather_only)],  # (a repeated target: GATHER only)
                         ids=lambda v: v if isinstance(v, str) else ("gather", "place")[v])
def test_cases(eng, torch, name, mode):
    c = case(name)
    got = run(eng, torch, c, mode)
    assert_digest(got, expected(c), set(listed(c).tolist()))


@pytest.mark.parametrize("name", [c.name for c in cases()])
def test_listed_documents_equal_the_full_digest_call(eng, torch, name):
    """Every case again, against crdt_awset_digest_async of the same replica on the device; PLACE too."""
    c = case(name)
    ds, dt = on_device(torch, c, GATHER)
    n = c.state.n_docs
    full = device_digest(torch, sentinel(n))
    eng.digest_async(ds, full, dt)
    eng.sync()
    rows = np.unique(listed(c).astype(np.int64))
    for mode in (GATHER,) if c.gather_only else (GATHER, PLACE):
        assert_digest(run(eng, torch, c, mode)[rows], read_digest(full, n)[rows])
    assert_digest(read_digest(full, n), full_digest(c))


def test_engine_digest_idx_host_wrapper(eng, torch):
    c = case("list_every_other")
    assert_digest(eng.digest_idx(c.state, c.idx, sentinel(c.state.n_docs), c.tombs), expected(c))
    sub, sub_t = place_sub(c)
    assert_digest(eng.digest_idx(sub, c.idx, sentinel(c.state.n_docs), sub_t, mode=PLACE), expected(c))
    # GATHER through the wrapper: a digest tensor that is not the replica's length is refused, not overrun
    ds, dt = on_device(torch, c, GATHER)
    short = device_digest(torch, sentinel(c.state.n_docs - 1))
    with pytest.raises(crdtgpu.CrdtError) as e:
        eng.digest_idx_async(ds, words(torch, c.idx), short, tombs=dt)
    assert e.value.code == CRDT_E_INVALID


# ------------------------------------------------------------------- 2. errors

def test_invalid_arguments(eng, torch):
    c = case("list_ascending")
    ds, dt = on_device(torch, c, GATHER)
    n = c.state.n_docs
    dig = device_digest(torch, sentinel(n))
    didx, dn = words(torch, c.idx), word(torch, n)
    lib, ctx = abi.lib(), eng._ctx
    cs, ct = ds.c(), dt.c()

    def rc(state=cs, tombs=ct, idx=didx.data_ptr(), n_idx=dn.data_ptr(), n_max=n, n_digest=n, mode=GATHER,
           digest=dig.data_ptr()):
        return lib.crdt_awset_digest_idx_async(ctx, ctypes.byref(state) if state is not None else None,
                                               ctypes.byref(tombs) if tombs is not None else None, idx, n_idx, n_max,
                                               n_digest, mode, digest, None)

    assert rc(state=None) == CRDT_E_INVALID
    assert rc(idx=None) == CRDT_E_INVALID
    assert rc(digest=None) == CRDT_E_INVALID
    for R in (0, 65):
        wide = ds.c()
        wide.R = R
        assert rc(state=wide) == CRDT_E_INVALID
    no_off = dt.c()
    no_off.offsets = None
    assert rc(tombs=no_off) == CRDT_E_INVALID
    assert rc(mode=2) == CRDT_E_INVALID
    assert rc(n_digest=n - 1) == CRDT_E_INVALID and rc(n_digest=n + 1) == CRDT_E_INVALID  # GATHER: == n_docs
    assert rc(mode=PLACE, n_max=n + 1, n_digest=4 * n) == CRDT_E_INVALID  # PLACE: state->n_docs >= n_max
    for arr in (ds.offsets, ds.keys, ds.actors, ds.counters, ds.vv, dt.offsets, dt.keys, dt.actors, dt.counters):
        assert rc(digest=arr.data_ptr()) == CRDT_E_INVALID  # digest starts where an input starts
        assert rc(idx=arr.data_ptr()) == CRDT_E_INVALID  # ... and so does the list
    assert rc(digest=didx.data_ptr()) == CRDT_E_INVALID and rc(digest=dn.data_ptr()) == CRDT_E_INVALID
    assert lib.crdt_awset_digest_idx_async(None, ctypes.byref(cs), None, didx.data_ptr(), None, n, n, GATHER,
                                           dig.data_ptr(), None) == CRDT_E_INVALID
    assert rc(n_max=0) == 0  # launches nothing
    eng.sync()
    assert_digest(read_digest(dig, n), sentinel(n))  # none of them wrote a word


@pytest.mark.parametrize("mode", [GATHER, PLACE], ids=["gather", "place"])
def test_n_idx_above_n_max_is_clamped(eng, torch, mode):
    c = case("list_descending")
    ds, dt = on_device(torch, c, mode)
    n, n_max = c.state.n_docs, 5
    dig = device_digest(torch, sentinel(n))
    eng.digest_idx_async(ds, words(torch, c.idx), dig, tombs=dt, n_idx=word(torch, n), n_max=n_max, mode=mode)
    assert _code(eng.sync) == CRDT_E_CAPACITY
    want = sentinel(n)
    rows = c.idx[:n_max].astype(np.int64)
    want[rows] = full_digest(c)[rows]
    assert_digest(read_digest(dig, n), want)  # the first n_max exact, nothing else written
    eng.sync()  # cleared


@pytest.mark.parametrize("mode", [GATHER, PLACE], ids=["gather", "place"])
def test_index_out_of_range_between_valid_neighbours(eng, torch, mode):
    c = case("list_ascending")
    ds, dt = on_device(torch, c, mode)
    n = c.state.n_docs
    for bad in (n, 2 ** 32 - 1):
        idx = c.idx.copy()
        idx[7] = bad
        dig = device_digest(torch, sentinel(n))
        eng.digest_idx_async(ds, words(torch, idx), dig, tombs=dt, mode=mode)
        assert _code(eng.sync) == CRDT_E_INVALID
        want = full_digest(c).copy()
        want[7] = sentinel(n)[7]  # nothing written for it; its neighbours exact
        assert_digest(read_digest(dig, n), want)


def test_live_count_above_its_slots_is_clamped(eng, torch):
    c = case("layout_slack_cont")  # the slack continues the document: the clamped count reads it as live
    n = c.state.n_docs
    d, dt_doc = MAIN_NAMES.index("ladder65"), MAIN_NAMES.index("ladder2")
    for which in ("entries", "tombs"):
        st = AWSetBatch(c.state.R, c.state.offsets, c.state.keys, c.state.actors, c.state.counters, c.state.vv,
                        counts=c.state.counts.copy())
        tb = TombBatch(c.tombs.offsets, c.tombs.keys, c.tombs.actors, c.tombs.counters, c.tombs.counts.copy())
        if which == "entries":
            st.counts[d] = int(st.offsets[d + 1] - st.offsets[d]) + 9
        else:
            tb.counts[dt_doc] = int(tb.offsets[dt_doc + 1] - tb.offsets[dt_doc]) + 1
        want = sentinel(n)
        want[:] = _clamped_host(st, tb)
        assert (want != full_digest(c)).any(axis=1).sum() == 1
        ds, dtb = upload(torch, st, tb)
        dig = device_digest(torch, sentinel(n))
        eng.digest_idx_async(ds, words(torch, c.idx), dig, tombs=dtb)
        assert _code(eng.sync) == CRDT_E_CAPACITY
        assert_digest(read_digest(dig, n), want)
    # PLACE: a packed sub-batch has no slack, so the clamped document is the document
    sub, sub_t = place_sub(c)
    sub = AWSetBatch(sub.R, sub.offsets, sub.keys, sub.actors, sub.counters, sub.vv, counts=sub.counts.copy())
    sub.counts[3] += 4
    ds, dtb = upload(torch, sub, sub_t)
    dig = device_digest(torch, sentinel(n))
    eng.digest_idx_async(ds, words(torch, c.idx), dig, tombs=dtb, mode=PLACE)
    assert _code(eng.sync) == CRDT_E_CAPACITY
    assert_digest(read_digest(dig, n), expected(c))


def _clamped_host(st, tb):
    """digest_host of the batch with every live count clamped to its slots (the host call refuses it unclamped)."""
    cl = lambda b: np.minimum(b.counts, np.diff(b.offsets.astype(np.int64)).astype(U32))  # noqa: E731
    return crdtgpu.digest_host(AWSetBatch(st.R, st.offsets, st.keys, st.actors, st.counters, st.vv, counts=cl(st)),
                               TombBatch(tb.offsets, tb.keys, tb.actors, tb.counters, cl(tb)))


# ------------------------------------------------------------------- 3. identity, streams, capture

@pytest.mark.parametrize("mode", [GATHER, PLACE], ids=["gather", "place"])
def test_run_to_run_identity(eng, torch, mode):
    c = case("list_descending")
    first = run(eng, torch, c, mode)
    for _ in range(3):
        assert (run(eng, torch, c, mode) == first).all()
    assert (run(eng, torch, c, mode, stream=torch.cuda.Stream()) == first).all()


def test_graph_capture_and_replay_after_the_state_and_n_idx_changed(eng, torch):
    """Captured on a fresh, unreserved context; replayed, then replayed again after the
    replica's contents, the list and *n_idx were overwritten in place."""
    c, c2 = case("list_every_other"), case("layout_counts")  # the same replica shape, counts given
    dev = dev_of(torch)
    n = c.state.n_docs
    ds, dt = upload(torch, c2.state, c2.tombs)
    m = n  # the list's capacity
    didx = torch.zeros(m, dtype=torch.int32, device=dev)
    didx[: len(c.idx)] = words(torch, c.idx)
    dn = word(torch, len(c.idx))
    dig = device_digest(torch, sentinel(n))
    e = crdtgpu.Engine(0)
    try:
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.digest_idx_async(ds, didx, dig, tombs=dt, n_idx=dn, n_max=m, stream=torch.cuda.current_stream())
        g.replay()
        e.sync(torch.cuda.current_stream())
        assert_digest(read_digest(dig, n), expected(c))
        # another state in the same arrays: every counter and clock word changed, the wave-bound
        # document cut short; another list and length
        st = c2.state
        counts = st.counts.copy()
        counts[MAIN_NAMES.index("wave+1")] = 77
        st2 = AWSetBatch(st.R, st.offsets, st.keys, st.actors, st.counters + U64(3), st.vv + U64(1), counts=counts)
        ds.counters.copy_(words64(torch, st2.counters))
        ds.vv.copy_(words64(torch, st2.vv))
        ds.counts.copy_(words(torch, st2.counts))
        idx2 = np.arange(n - 1, -1, -1).astype(U32)
        didx.copy_(words(torch, idx2))
        dn.fill_(n - 3)
        dig.copy_(device_digest(torch, sentinel(n)))
        g.replay()
        e.sync(torch.cuda.current_stream())
        want = sentinel(n)
        rows = idx2[: n - 3].astype(np.int64)
        want[rows] = crdtgpu.digest_host(st2, c2.tombs)[rows]
        assert (want[rows] != expected(case("list_descending"))[rows]).any(axis=1).all()
        assert_digest(read_digest(dig, n), want)
    finally:
        e.close()


def words64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, U64).view(np.int64).copy()).to(dev_of(torch))


# ------------------------------------------------------------------- 4. the round

_round = {}


def round_model():
    """A replica of 600 documents repacked with headroom, local ops on every 20th document (5 %):
    the selection, the ops, and the host replica the in-place scatter leaves."""
    if not _round:
        from oracle import oracle

        rep0, idx, part, _ = apply_round_case(every=20)
        p = replica_select_ref(rep0).rep
        roomy = replica_repack_ref(Replica(p.state, p.tombs, 0, p.doc_actor), er=ROUND_ROOM, tr=ROUND_ROOM).rep
        s = replica_select_ref(roomy, idx, n_out=len(idx)).rep
        rc, out, tout = oracle.apply(s.state, part, s.tombs)
        assert rc == 0
        sub = Replica(out.as_batch(), tout, 0, s.doc_actor)
        ref = replica_scatter_inplace_ref(roomy, sub, idx)
        assert len(ref.spill_j) == 0 and len(ref.placed_j) == len(idx)  # with headroom everything fits
        _round.update(roomy=roomy, idx=idx, part=part, after=ref.rep)
    return _round


def test_sparse_apply_round_keeps_the_digest_array_current(eng, torch):
    """full digest once; select, apply, [PLACE: digest_idx of the apply output], in-place
    scatter, [GATHER: digest_idx of the replica]: either array is the full digest of the new
    replica, with no second pass over the replica."""
    dev = dev_of(torch)
    m = round_model()
    rep, idx, part, after = m["roomy"], m["idx"], m["part"], m["after"]
    n, R, k = rep.n_docs, rep.state.R, len(idx)
    assert 300 <= n <= 1000 and k * 20 == n
    before = crdtgpu.digest_host(rep.state, rep.tombs)
    want = crdtgpu.digest_host(after.state, after.tombs)
    changed = (before != want).any(axis=1)
    assert changed.sum() >= k // 2 and not changed[np.setdiff1d(np.arange(n), idx)].any()
    dr, didx = rep.to(dev), words(torch, idx)
    dig_gather = torch.empty(2 * n, dtype=torch.int64, device=dev)
    eng.digest_async(dr.state, dig_gather, dr.tombs)
    eng.sync()
    assert_digest(read_digest(dig_gather, n), before)
    dig_place = dig_gather.clone()
    torch.cuda.synchronize()
    e_sel, t_sel = int(rep.state.offsets[-1]), int(rep.tombs.offsets[-1])
    pops = int(part.op_off[-1])
    sel = ReplicaBuffers(k, R, e_sel, t_sel, device=dev)
    eng.replica_select_async(dr, sel, didx, None, k)
    so, st = OutBuffers(k, R, e_sel + pops, device=dev), TombBuffers(k, t_sel + pops, device=dev)
    dpart = part.to(dev)
    dpart.doc_actor = sel.doc_actor
    eng.apply_async(sel.state.as_batch(), dpart, so, sel.tombs, st)
    # PLACE: from the merged selection, before the scatter
    eng.digest_idx_async(so.as_batch(), didx, dig_place, tombs=st, mode=PLACE)
    sp = SpillBuffers(k, device=dev)
    eng.replica_scatter_inplace_async(dr, Replica(so.as_batch(), st, 0, sel.doc_actor), didx, sp)
    # GATHER: from the replica, after the scatter
    eng.digest_idx_async(dr.state, didx, dig_gather, tombs=dr.tombs)
    eng.sync()
    assert int(_np(sp.n_spill, U32)[0]) == 0
    assert_digest(read_digest(dig_place, n), want)
    assert_digest(read_digest(dig_gather, n), want)
