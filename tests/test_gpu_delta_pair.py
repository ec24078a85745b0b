"""GPU: crdt_awset_delta_join_async / crdt_awset_delta_exchange_async
(csrc/delta_pair.hip) against delta_pair_ref (tests/delta_pair_cases.py, pinned by
tests/test_delta_pair_model.py): entries, counts, offsets, clocks and kinds,
bit-exact, in both directions.

Every output buffer is pre-filled with poison, so each word compared was written
by the call.  The wave path takes a document whose two sides hold at most 64 live
entries and 64 live tombstones each (kPairWaveMax), four documents per workgroup
(kPairWaves); the rest goes through the worklist to the block path, which steps
a window of 1,024 merged positions.  No test provokes a fault: the error cases
are the clamped, reported ones of the contract.
"""

import ctypes
import json
import random

import numpy as np
import pytest

import crdtgpu
from apply_cases import encode, make_case
from counter_maps import assert_mixes, map_batch, map_out, mixed
from crdtgpu import (CRDT_DELTA_DELTA, CRDT_DELTA_FULL, CRDT_DELTA_NONE, CRDT_E_ACTOR_RANGE, CRDT_E_CAPACITY,
                     CRDT_E_INVALID, CRDT_E_WORKSPACE, abi)
from crdtgpu.batch import AWSetBatch, CompareBuffers, OpBatch, OutBuffers, Replica, TombBatch, TombBuffers
from delta_pair_cases import (MAX_C, PAIR_WAVES, assert_direction, delta_pair_ref, edge_pair, on_wave_path, pair_docs,
                              phase2_doc, random_pair)
from helpers import GOLDEN, out_doc
from sources_cases import LAYOUTS, make_replica
from test_compare_model import compare_ref
from test_gpu_compare import _code, dev_of, host_out, poisoned_out

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
POISON_KIND = 77


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

def slots_of(a, b):
    return int(a.state.offsets[-1]) + int(b.state.offsets[-1])


def kind_buf(torch, n):
    return torch.full((max(n, 1),), POISON_KIND, dtype=torch.uint8, device=dev_of(torch))


def kinds_host(t, n):
    return t.cpu().numpy().view(U8)[:n]


def exchange_on_device(eng, torch, a, b, da=None, db=None, stream=None):
    """(out_ab, out_ba, kind_ab, kind_ba) on the device after one call; not synced."""
    n, R = a.n_docs, a.state.R
    dev = dev_of(torch)
    o1, o2 = poisoned_out(torch, n, R, slots_of(a, b)), poisoned_out(torch, n, R, slots_of(a, b))
    k1, k2 = kind_buf(torch, n), kind_buf(torch, n)
    eng.delta_exchange_async(da or a.to(dev), db or b.to(dev), o1, o2, k1, k2, stream=stream)
    return o1, o2, k1, k2


def assert_pair(got, a, b, want=None):
    """A device exchange result equals delta_pair_ref(a, b)."""
    want = want or delta_pair_ref(a, b)
    assert want.rc_ab == 0 and want.rc_ba == 0
    o1, o2, k1, k2 = got
    n = a.n_docs
    h1, h2 = host_out(o1), host_out(o2)
    assert_direction(h1, want.ab, a.state, b.state, "a <- b")
    assert_direction(h2, want.ba, a.state, b.state, "b <- a")
    for name, g, w in (("kind_ab", kinds_host(k1, n), want.kind_ab), ("kind_ba", kinds_host(k2, n), want.kind_ba)):
        if not (g == w).all():
            d = int(np.nonzero(g != w)[0][0])
            raise AssertionError("%s differs first at document %d: gpu %d, expected %d" % (name, d, g[d], w[d]))
    return h1, h2, want


def check_exchange(eng, torch, a, b):
    got = exchange_on_device(eng, torch, a, b)
    eng.sync()
    return assert_pair(got, a, b)


def same_docs(x, y, n, R, docs=None):
    for d in (range(n) if docs is None else docs):
        assert out_doc(x, d, R) == out_doc(y, d, R), d


def host_state(out):
    h = host_out(out)
    return AWSetBatch(out.R, h.offsets, h.keys, h.actors, h.counters, h.vv, counts=h.counts)


# ------------------------------------------------------------ 1. random parity

@pytest.mark.parametrize("R", [1, 2, 5, 64])
def test_random_parity(eng, torch, R):
    """3,000 small documents (the set tests/test_delta_pair_model.py takes the census of);
    each direction's delta_join_async equals its half of the exchange; a FULL document
    equals crdt_awset_join_async's output for it."""
    a, b = random_pair(6000 + R, 3000, R)
    n = a.n_docs
    h1, h2, want = check_exchange(eng, torch, a, b)
    dev = dev_of(torch)
    da, db = a.to(dev), b.to(dev)
    for dst, src, half, kinds in ((da, db, h1, want.kind_ab), (db, da, h2, want.kind_ba)):
        o, k = poisoned_out(torch, n, R, slots_of(a, b)), kind_buf(torch, n)
        eng.delta_join_async(dst.state, src, o, k)
        eng.sync()
        h = host_out(o)
        same_docs(h, half, n, R)
        assert (h.offsets[: n + 1] == half.offsets[: n + 1]).all() and (h.counts[:n] == half.counts[:n]).all()
        assert (kinds_host(k, n) == kinds).all()
        oj = poisoned_out(torch, n, R, slots_of(a, b))
        eng.join_async(dst.state, src.state, oj)
        eng.sync()
        full = np.nonzero(kinds == CRDT_DELTA_FULL)[0].tolist()
        assert len(full) > n // 10
        same_docs(host_out(oj), h, n, R, full)


# ------------------------------------------------------------ 2. dispatch edges

@pytest.fixture(scope="module")
def edges():
    da, db = edge_pair()
    a, b = make_replica(2, da, actor=0), make_replica(2, db, actor=1)
    return a, b, delta_pair_ref(a, b)


def test_dispatch_edges(eng, torch, edges):
    """0, 1, 63, 64, 65 and 129 entries a side and 0, 1, 64 and 65 tombstones, every
    combination that changes the path, in all three kinds; documents of 3,000 entries
    a side step the block path's window; n_docs is no multiple of the workgroup's four."""
    a, b, want = edges
    assert a.n_docs % PAIR_WAVES != 0
    got = exchange_on_device(eng, torch, a, b)
    eng.sync()
    assert_pair(got, a, b, want)


@pytest.mark.parametrize("which", ["wave", "block"])
def test_one_document(eng, torch, which):
    rng = random.Random(6100)
    x, y = pair_docs(rng, 2, 7, 5, 2, 3, 1) if which == "wave" else pair_docs(rng, 2, 130, 70, 3, 66, 1)
    a, b = make_replica(2, [x], actor=0), make_replica(2, [y], actor=1)
    assert on_wave_path(a, b, 0) == (which == "wave")
    check_exchange(eng, torch, a, b)


# ------------------------------------------------------------------ 3. layouts

def _layout(i, seed):
    lay = dict(LAYOUTS[i])
    if lay.pop("garbage", False):
        lay["garbage"] = np.random.default_rng(seed)
    return lay


@pytest.mark.parametrize("la,lb", [(3, 0), (1, 2), (2, 3), (0, 1)])
def test_slot_layouts(eng, torch, la, lb):
    """Slack with stale values behind the live prefixes, counts given and NULL, the two
    replicas laid out independently, a lead before the first document."""
    a, b = random_pair(6200 + la, 1000, 3, max_e=70, max_t=70, lay_a=dict(_layout(la, 1), lead=la),
                       lay_b=dict(_layout(lb, 2), lead=2 * lb))
    assert sum(not on_wave_path(a, b, d) for d in range(a.n_docs)) > 20
    check_exchange(eng, torch, a, b)


@pytest.mark.parametrize("ta,tb", [(False, True), (True, False), (False, False)])
def test_without_tombstones(eng, torch, ta, tb):
    a, b = random_pair(6300, 1000, 2, max_e=70, tombs_a=ta, tombs_b=tb)
    assert (a.tombs is None) == (not ta) and (b.tombs is None) == (not tb)
    check_exchange(eng, torch, a, b)


def test_actor_per_document_and_scalar(eng, torch):
    a, b = random_pair(6400, 1000, 5, max_e=70, doc_actors=True)
    assert a.doc_actor is not None and len(set(a.doc_actor.tolist())) == 5
    h1, h2, want = check_exchange(eng, torch, a, b)
    assert len(set(want.kind_ab.tolist())) == 3
    # one actor for all: the scalar and the array forms agree
    for r in (a, b):
        r.doc_actor[:] = 3
    h1, h2, _ = check_exchange(eng, torch, a, b)
    sa, sb = Replica(a.state, a.tombs, actor=3), Replica(b.state, b.tombs, actor=3)
    g1, g2, _ = check_exchange(eng, torch, sa, sb)
    same_docs(g1, h1, a.n_docs, 5)
    same_docs(g2, h2, a.n_docs, 5)


def test_exchange_output_is_an_input_as_it_stands(eng, torch):
    """Documents at capacity offsets: the outputs of one exchange, on the device, are the
    states of the next (each side's tombstones unchanged: a merge writes none)."""
    a, b = random_pair(6500, 1000, 3, max_e=70, max_t=70)
    dev = dev_of(torch)
    da, db = a.to(dev), b.to(dev)
    o1, o2, _, _ = exchange_on_device(eng, torch, a, b, da, db)
    a2d, b2d = Replica(o1.as_batch(), da.tombs, actor=a.actor), Replica(o2.as_batch(), db.tombs, actor=b.actor)
    n, R = a.n_docs, 3
    p1, p2 = poisoned_out(torch, n, R, 2 * slots_of(a, b)), poisoned_out(torch, n, R, 2 * slots_of(a, b))
    k1, k2 = kind_buf(torch, n), kind_buf(torch, n)
    eng.delta_exchange_async(a2d, b2d, p1, p2, k1, k2)
    eng.sync()
    a2, b2 = Replica(host_state(o1), a.tombs, actor=a.actor), Replica(host_state(o2), b.tombs, actor=b.actor)
    assert int(a2.state.offsets[-1]) > int(a2.state.counts.sum())  # capacity offsets: slack behind the live prefixes
    assert_pair((p1, p2, k1, k2), a2, b2)


# ------------------------------------------------------------------- 4. errors

def small_pair(R=2):
    x, y = phase2_doc(R)
    rng = random.Random(6600)
    docs = [pair_docs(rng, R, 4, 5, 1, 2, m) for m in (0, 1, 2)] + [(x, y)]
    return [p[0] for p in docs], [p[1] for p in docs]


def test_actor_range_on_the_path_select(eng, torch):
    """Counter(s) at s == R is the reference's panic; s > R is "never seen": FULL."""
    da, db = small_pair()
    a, b = make_replica(2, da, actor=0), make_replica(2, db, actor=2)
    exchange_on_device(eng, torch, a, b)
    assert _code(eng.sync) == CRDT_E_ACTOR_RANGE
    eng.sync()  # cleared
    a, b = make_replica(2, da, actor=0), make_replica(2, db, actor=3)
    h1, _, want = check_exchange(eng, torch, a, b)
    assert (want.kind_ab == CRDT_DELTA_FULL).all()
    a, b = make_replica(2, da, actor=0), make_replica(2, db, actor=0, doc_actor=[0, 1, 2, 1])
    exchange_on_device(eng, torch, a, b)
    assert _code(eng.sync) == CRDT_E_ACTOR_RANGE


@pytest.mark.parametrize("size", [3, 80])
def test_actor_range_on_a_has_dot(eng, torch, size):
    """A src entry dot with actor == R on the DELTA path (HasDot against dst's clock),
    at wave and at block size; the oracle reports the same."""
    rng = random.Random(6700 + size)
    x, y = pair_docs(rng, 2, size, size, 0, 0, 1)
    y = ([(k, 2, c) if i == 1 else (k, a_, c) for i, (k, a_, c) in enumerate(y[0])], y[1], y[2])
    a, b = make_replica(2, [x], actor=0), make_replica(2, [y], actor=1)
    want = delta_pair_ref(a, b)
    assert want.rc_ab == CRDT_E_ACTOR_RANGE and int(want.kind_ab[0]) != CRDT_DELTA_FULL
    dev = dev_of(torch)
    o, k = poisoned_out(torch, 1, 2, slots_of(a, b)), kind_buf(torch, 1)
    eng.delta_join_async(a.to(dev).state, b.to(dev), o, k)
    assert _code(eng.sync) == CRDT_E_ACTOR_RANGE
    # actor > R in the same place is "never seen": no error
    y2 = ([(k_, 3, c) if a_ == 2 else (k_, a_, c) for k_, a_, c in y[0]], y[1], y[2])
    b2 = make_replica(2, [y2], actor=1)
    check_exchange(eng, torch, a, b2)


@pytest.mark.parametrize("which", ["entries", "tombstones"])
def test_count_above_slots_is_clamped(eng, torch, which):
    da, db = small_pair()
    a = make_replica(2, da, actor=0, slack=1, with_counts=True)
    b = make_replica(2, db, actor=1, slack=1, with_counts=True)
    cols = b.state if which == "entries" else b.tombs
    cols.counts[1] = int(cols.offsets[2]) - int(cols.offsets[1]) + 9
    got = exchange_on_device(eng, torch, a, b)
    assert _code(eng.sync) == CRDT_E_CAPACITY
    eng.sync()  # cleared
    # the other documents are what they would be without the bad count
    cols.counts[1] = int(cols.offsets[2]) - int(cols.offsets[1]) - 1
    want = delta_pair_ref(a, b)
    h1, h2 = host_out(got[0]), host_out(got[1])
    same_docs(h1, want.ab, 4, 2, [0, 2, 3])
    same_docs(h2, want.ba, 4, 2, [0, 2, 3])


@pytest.mark.parametrize("which", ["entries", "tombstones"])
def test_count_above_slots_is_clamped_at_block_size(eng, torch, which):
    """The same with 70 entries and 70 tombstones a side: the documents are the block
    path's, which clamps the count again."""
    rng = random.Random(6800)
    docs = [pair_docs(rng, 2, 70, 70, 70, 70, m) for m in (0, 1, 2)]
    a = make_replica(2, [p[0] for p in docs], actor=0, slack=1, with_counts=True)
    b = make_replica(2, [p[1] for p in docs], actor=1, slack=1, with_counts=True)
    assert not on_wave_path(a, b, 1)
    cols = b.state if which == "entries" else b.tombs
    cols.counts[1] = int(cols.offsets[2]) - int(cols.offsets[1]) + 9
    got = exchange_on_device(eng, torch, a, b)
    assert _code(eng.sync) == CRDT_E_CAPACITY
    eng.sync()  # cleared
    cols.counts[1] = int(cols.offsets[2]) - int(cols.offsets[1]) - 1
    want = delta_pair_ref(a, b)
    h1, h2 = host_out(got[0]), host_out(got[1])
    same_docs(h1, want.ab, 3, 2, [0, 2])
    same_docs(h2, want.ba, 3, 2, [0, 2])


def test_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched."""
    da, db = small_pair()
    dev = dev_of(torch)
    a, b = make_replica(2, da, actor=0).to(dev), make_replica(2, db, actor=1).to(dev)
    b3 = make_replica(2, db[:3], actor=1).to(dev)
    da3, db3 = small_pair(3)
    bR = make_replica(3, db3, actor=1).to(dev)
    n, R, slots = 4, 2, 64
    o1, o2 = poisoned_out(torch, n, R, slots), poisoned_out(torch, n, R, slots)
    k1, k2 = kind_buf(torch, n), kind_buf(torch, n)
    lib, ctx, ref = abi.lib(), eng._ctx, ctypes.byref

    def xchg(ca, cb, c1, c2, p1=None, p2=None):
        return lib.crdt_awset_delta_exchange_async(ctx, ref(ca) if ca else None, ref(cb) if cb else None,
                                                   ref(c1) if c1 else None, ref(c2) if c2 else None, p1, p2, None)

    def join(cd, cs, co, p=None):
        return lib.crdt_awset_delta_join_async(ctx, ref(cd) if cd else None, ref(cs) if cs else None,
                                               ref(co) if co else None, p, None)

    ca, cb = a.c(), b.c()
    assert xchg(None, cb, o1.c(), o2.c()) == CRDT_E_INVALID
    assert xchg(ca, None, o1.c(), o2.c()) == CRDT_E_INVALID
    assert xchg(ca, cb, None, o2.c()) == CRDT_E_INVALID
    assert xchg(ca, cb, o1.c(), None) == CRDT_E_INVALID
    assert join(None, cb, o1.c()) == CRDT_E_INVALID
    assert join(a.state.c(), None, o1.c()) == CRDT_E_INVALID
    assert join(a.state.c(), cb, None) == CRDT_E_INVALID
    assert xchg(ca, b3.c(), o1.c(), o2.c()) == CRDT_E_INVALID  # n_docs
    assert xchg(ca, bR.c(), o1.c(), o2.c()) == CRDT_E_INVALID  # R
    assert join(a.state.c(), bR.c(), o1.c()) == CRDT_E_INVALID
    no_state = b.c()
    no_state.state = None
    assert xchg(ca, no_state, o1.c(), o2.c()) == CRDT_E_INVALID
    wide_state = a.state.c()
    wide_state.R = 65
    wide = abi.CReplica(ctypes.addressof(wide_state), None, None, 0)
    assert xchg(wide, wide, o1.c(), o2.c()) == CRDT_E_INVALID  # R out of range
    no_off = b.tombs.c()
    no_off.offsets = None
    cs = b.state.c()
    bad_t = abi.CReplica(ctypes.addressof(cs), ctypes.addressof(no_off), None, 1)
    assert xchg(ca, bad_t, o1.c(), o2.c()) == CRDT_E_INVALID  # a tomb batch without offsets
    assert join(a.state.c(), bad_t, o1.c()) == CRDT_E_INVALID
    for f in ("offsets", "counts", "keys", "actors", "counters", "vv"):
        c = o1.c()
        setattr(c, f, None)
        assert xchg(ca, cb, c, o2.c()) == CRDT_E_INVALID, f
        assert xchg(ca, cb, o2.c(), c) == CRDT_E_INVALID, f
        assert join(a.state.c(), cb, c) == CRDT_E_INVALID, f
        # the two directions share no array, the key column included
        c = o2.c()
        setattr(c, f, getattr(o1.c(), f))
        assert xchg(ca, cb, o1.c(), c) == CRDT_E_INVALID, f
    for f, g in (("keys", "counters"), ("offsets", "counts"), ("keys", "vv")):
        c = o1.c()
        setattr(c, f, getattr(o2.c(), g))
        assert xchg(ca, cb, c, o2.c()) == CRDT_E_INVALID, (f, g)
    # an output array starting where an input array of the same kind starts
    for f, src in (("keys", a.state.keys), ("counters", b.state.keys), ("vv", b.state.vv), ("actors", a.state.actors),
                   ("offsets", b.state.offsets), ("keys", b.tombs.keys), ("counters", a.tombs.counters),
                   ("actors", b.tombs.actors), ("counts", b.tombs.offsets)):
        c = o1.c()
        setattr(c, f, src.data_ptr())
        assert xchg(ca, cb, c, o2.c()) == CRDT_E_INVALID, f
        assert xchg(ca, cb, o2.c(), c) == CRDT_E_INVALID, f
    c = o1.c()
    c.keys = b.state.keys.data_ptr()
    assert join(a.state.c(), cb, c) == CRDT_E_INVALID
    assert xchg(ca, cb, o1.c(), o2.c(), k1.data_ptr(), k1.data_ptr()) == CRDT_E_INVALID  # one kind array for both
    eng.sync()
    for o in (o1, o2):
        for t in (o.offsets, o.counts, o.actors):
            assert (t.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
        for t in (o.keys, o.counters, o.vv):
            assert (t.cpu().numpy().view(U64) == 2 ** 64 - 1).all()
    assert (kinds_host(k1, n) == POISON_KIND).all()
    # kind is optional, and the call still works
    eng.delta_exchange_async(a, b, o1, o2)
    eng.delta_join_async(a.state, b, poisoned_out(torch, n, R, slots))
    eng.sync()


def test_no_documents(eng, torch):
    dev = dev_of(torch)
    z = lambda dt: torch.zeros(1, dtype=dt, device=dev)  # noqa: E731
    st = AWSetBatch(2, z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64))
    e = Replica(st, TombBatch(z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64)), actor=1)
    assert e.n_docs == 0
    o1, o2 = poisoned_out(torch, 1, 2, 4), poisoned_out(torch, 1, 2, 4)
    k = kind_buf(torch, 0)
    eng.delta_exchange_async(e, e, o1, o2, k, None)
    eng.delta_join_async(st, e, o1, k)
    eng.sync()
    for o in (o1, o2):
        assert (o.keys.cpu().numpy().view(U64) == 2 ** 64 - 1).all() and int(o.counts.cpu().numpy().view(U32)[0]) == 2 ** 32 - 1
    assert int(k.cpu().numpy()[0]) == POISON_KIND


def test_graph_capture(torch):
    """Captured on a reserved context, replayed twice with the inputs changed in between,
    equal to eager; on an unreserved context the capture is refused with
    CRDT_E_WORKSPACE and launches nothing."""
    a, b = random_pair(6800, 1500, 2, max_e=70, max_t=3)
    n, R = a.n_docs, 2
    assert n > 1024  # (a fresh context's workspace holds 1,024 documents)
    assert sum(not on_wave_path(a, b, d) for d in range(n)) > 20
    dev = dev_of(torch)
    slots = slots_of(a, b)
    e = crdtgpu.Engine(0)
    try:
        da, db = a.to(dev), b.to(dev)
        o1, o2 = poisoned_out(torch, n, R, slots), poisoned_out(torch, n, R, slots)
        k1, k2 = kind_buf(torch, n), kind_buf(torch, n)
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.delta_exchange_async(da, db, o1, o2, k1, k2, stream=torch.cuda.current_stream())
        assert ei.value.code == CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        assert (kinds_host(k1, n) == POISON_KIND).all() and (o1.counts.cpu().numpy().view(U32) == 2 ** 32 - 1).all()
        e.reserve(n)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.delta_exchange_async(da, db, o1, o2, k1, k2, stream=torch.cuda.current_stream())
        for vv_src in (b, a, b):  # the clocks of b change between replays: other kinds, other survivors
            db.state.vv.copy_(vv_src.state.to(dev).vv)
            hb = Replica(AWSetBatch(R, b.state.offsets, b.state.keys, b.state.actors, b.state.counters, vv_src.state.vv),
                         b.tombs, actor=b.actor)
            for o in (o1, o2):
                for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
                    t.fill_(-1)
            k1.fill_(POISON_KIND)
            k2.fill_(POISON_KIND)
            g.replay()
            e.sync(torch.cuda.current_stream())
            assert_pair((o1, o2, k1, k2), a, hb)
            eager = exchange_on_device(e, torch, a, hb)
            e.sync()
            for x, y in zip((o1, o2), eager[:2]):
                hx, hy = host_out(x), host_out(y)
                same_docs(hx, hy, n, R)
                assert (hx.counts == hy.counts).all() and (hx.offsets == hy.offsets).all()
    finally:
        e.close()


# ------------------------------------------------------------ 5. wide counters

def _mapped(rep, tab):
    return Replica(map_batch(rep.state, tab), map_batch(rep.tombs, tab) if rep.tombs is not None else None,
                   actor=rep.actor, doc_actor=rep.doc_actor)


@pytest.mark.parametrize("case", ["edges", "random"])
def test_wide_counters(eng, torch, edges, case):
    """The same documents with every counter and clock value through the
    order-preserving maps of tests/counter_maps.py (up to 2^32, 2^63, 2^64 - 1): equal
    to the oracle on the mapped inputs, and to the mapped result of the unmapped run."""
    if case == "edges":
        a, b, want = edges
    else:
        a, b = random_pair(6900, 2000, 5, max_e=70, max_t=8)
        want = delta_pair_ref(a, b)
    period = 3  # pair_docs' modes cycle over d: the map also advances once per cycle
    tab = mixed(MAX_C, period)
    am, bm = _mapped(a, tab), _mapped(b, tab)
    h1, h2, want_m = check_exchange(eng, torch, am, bm)
    assert_mixes(want_m.ab, tab, "a <- b")
    assert_mixes(want_m.ba, tab, "b <- a")
    assert (want_m.kind_ab == want.kind_ab).all() and (want_m.kind_ba == want.kind_ba).all()
    n, R = a.n_docs, a.state.R
    for got, plain in ((h1, want.ab), (h2, want.ba)):
        m = map_out(plain, tab)
        same_docs(got, m, n, R)


# ------------------------------------------------------------- 6. composition

def test_apply_exchange_compare_on_the_device(eng, torch):
    """apply (Add, Del, AWSetDelta.Del) on both replicas -> delta exchange -> compare,
    with nothing downloaded in between; each stage's output is the next one's input
    as it stands."""
    rng = random.Random(7000)
    n, R = 1500, 3
    dev = dev_of(torch)
    sides = []
    for p in range(2):
        st, tb, ops, want = make_case(rng, n, R, lambda: rng.randint(0, 12), lambda: rng.randint(0, 10), universe=40,
                                      max_c=MAX_C)
        assert all(w is not None for w in want)
        nops = int(ops.op_off[-1])
        out = OutBuffers(n, R, int(st.offsets[-1]) + nops, device=dev)
        tout = TombBuffers(n, int(tb.offsets[-1]) + nops, device=dev)
        dops = ops.to(dev)
        eng.apply_async(st.to(dev), dops, out, tb.to(dev), tout)
        sides.append(dict(out=out, tout=tout, dops=dops, ops=ops, want=want))
    ra = Replica(sides[0]["out"].as_batch(), sides[0]["tout"], doc_actor=sides[0]["dops"].doc_actor)
    rb = Replica(sides[1]["out"].as_batch(), sides[1]["tout"], doc_actor=sides[1]["dops"].doc_actor)
    slots = sides[0]["out"].slots + sides[1]["out"].slots
    o1, o2 = poisoned_out(torch, n, R, slots), poisoned_out(torch, n, R, slots)
    k1, k2 = kind_buf(torch, n), kind_buf(torch, n)
    eng.delta_exchange_async(ra, rb, o1, o2, k1, k2)
    res = CompareBuffers(n, device=dev)
    eng.compare_async(o1.as_batch(), o2.as_batch(), res)
    eng.sync()
    # expected from the reference's own ops (apply_cases.replay), then delta_pair_ref
    host = []
    for s in sides:
        docs = [(w[0], w[1], w[2]) for w in s["want"]]
        host.append(make_replica(R, docs, doc_actor=s["ops"].doc_actor))
    ha = Replica(host_state(sides[0]["out"]), host[0].tombs, doc_actor=host[0].doc_actor)
    hb = Replica(host_state(sides[1]["out"]), host[1].tombs, doc_actor=host[1].doc_actor)
    for d in range(0, n, 7):  # the applied states are the reference's
        assert ha.state.doc(d) == (host[0].state.doc(d)) and hb.state.doc(d) == host[1].state.doc(d)
    _, _, want = assert_pair((o1, o2, k1, k2), ha, hb)
    assert len(set(want.kind_ab.tolist())) >= 2
    flags, summary, work = res.numpy()
    wf, ws, ww = compare_ref(want.ab.as_batch(), want.ba.as_batch())
    assert (flags == wf).all() and (summary == ws).all() and (work == ww).all()


# -------------------------------------------------------------------- 7. KAT-5

def test_kat5_on_resident_replicas(eng, torch):
    """TestAWSetDelta (awset-delta_test.go:168-189) from tests/golden/kat_scenarios.json:
    both replicas stay on the device, every Add / Del is an apply and every Merge a
    delta_join_async.  The element sets equal the golden ones at every assertEntries
    and every recorded state, including the step whose no-op delta leaves A's clock
    at [5, 2] while B's is [5, 3]."""
    sc = [s for s in json.load(open(GOLDEN))["scenarios"] if s["name"].startswith("KAT-5")][0]
    names = sorted({k for st in sc["steps"] if st[0] in ("add", "del") for k in st[2]})
    ids = {k: i + 1 for i, k in enumerate(names)}
    R = 2
    dev = dev_of(torch)

    def empty(actor):
        z = np.zeros(1, U64)
        st = AWSetBatch(R, np.zeros(2, U32), z, np.zeros(1, U32), z.copy(), np.zeros(R, U64)).to(dev)
        tb = TombBatch.from_lists([[]]).to(dev)
        return dict(state=st, tombs=tb, actor=actor, slots=0, tslots=0)

    reps = {"A": empty(0), "B": empty(1)}

    def snapshot(r):
        s = r["state"]
        h = AWSetBatch(R, *(t.cpu().numpy().view(U32 if t.dtype == torch.int32 else U64)
                            for t in (s.offsets, s.keys, s.actors, s.counters, s.vv)),
                       counts=None if s.counts is None else s.counts.cpu().numpy().view(U32))
        return h.doc(0)

    def apply(r, calls):
        ops = OpBatch.from_lists([encode(calls)], [r["actor"]])
        nops = int(ops.op_off[-1])
        out = OutBuffers(1, R, r["slots"] + nops, device=dev)
        tout = TombBuffers(1, r["tslots"] + nops, device=dev)
        eng.apply_async(r["state"], ops.to(dev), out, r["tombs"], tout)
        r.update(state=out.as_batch(), tombs=tout, slots=out.slots, tslots=r["tslots"] + nops)

    kinds = []
    for st in sc["steps"]:
        op, who = st[0], st[1]
        r = reps[who]
        if op == "add":
            apply(r, [("add", [ids[k] for k in st[2]])])
        elif op == "del":
            apply(r, [("ddel", [ids[k] for k in st[2]])])
        elif op == "merge":
            src = reps[st[2]]
            out = OutBuffers(1, R, r["slots"] + src["slots"], device=dev)
            k = kind_buf(torch, 1)
            eng.delta_join_async(r["state"], Replica(src["state"], src["tombs"], actor=src["actor"]), out, k)
            eng.sync()
            kinds.append(int(k.cpu().numpy()[0]))
            r.update(state=out.as_batch(), slots=out.slots)
        elif op == "expect":
            eng.sync()
            e, vv = snapshot(r)
            assert e == sorted((ids[k], d[0], d[1]) for k, d in st[2].items()), (who, st)
            assert vv == st[3], (who, st)
        elif op == "assert_entries":
            eng.sync()
            e, _ = snapshot(r)
            assert [k for k, _, _ in e] == sorted(ids[k] for k in st[2]), (who, st)
        else:
            raise AssertionError(op)
    assert kinds == [CRDT_DELTA_FULL, CRDT_DELTA_FULL, CRDT_DELTA_DELTA, CRDT_DELTA_NONE]
    eng.sync()
    for who, want in sc["final"].items():
        e, vv = snapshot(reps[who])
        assert vv == want["vv"] and e == sorted((ids[k], a_, c) for k, a_, c in want["entries"]), who
    assert snapshot(reps["A"])[1] == [5, 2] and snapshot(reps["B"])[1] == [5, 3]
