"""GPU: crdt_awset_delta_extract_* (csrc/extract.hip) against the restatement
of tests/test_delta_extract_model.py -- every source's kind, entries,
tombstones, actor and clock bit-exact, the packed offsets equal to the running
sums -- and through the existing CRDT_FOLD_DELTA fold: folding the message
gives what folding the full states gives, for an exact and for a stale peer
clock.

The scan over groups of 64 / R documents runs in chunks of 8,192 groups
(pack.hip's form), so the chunk edges are at n_docs = 8,192 * (64 / R) +- 1.
"""

import random

import numpy as np
import pytest

import crdtgpu
import test_delta_extract_model as model
from crdtgpu import CRDT_FOLD_DELTA
from crdtgpu.batch import SrcBatch, SrcBuffers
from helpers import batch_of, out_doc, random_state, ref, src_batch_of
from test_delta_extract_model import DELTA, FULL, NONE

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


# ---------------------------------------------------------------- helpers

def device_buffers(torch, srcs):
    """(device copy of host sources, output buffers of the input's capacity, kind)."""
    dev = torch.device("cuda:0")
    ns = srcs.n_srcs
    ne = int(srcs.entry_off[ns])
    nt = int(srcs.tomb_off[ns]) if srcs.tomb_off is not None else 0
    out = SrcBuffers(srcs.R, srcs.n_docs, ns, ne, nt, device=dev)
    for f, _ in SrcBatch._FIELDS:  # poison: everything read back must have been written
        getattr(out, f).fill_(-1)
    kind = torch.full((max(ns, 1),), 77, dtype=torch.uint8, device=dev)
    return srcs.to(dev), out, kind


def to_dev(torch, a):
    a = np.ascontiguousarray(a, dtype=U64)
    return torch.from_numpy(np.concatenate([a, np.zeros(1, U64)]).view(np.int64)).to("cuda:0")


def extract(eng, torch, srcs, peer):
    ds, out, kind = device_buffers(torch, srcs)
    eng.delta_extract_async(ds, to_dev(torch, peer), out, kind=kind)
    eng.sync()
    torch.cuda.synchronize()
    return out.numpy(), kind.cpu().numpy()[: srcs.n_srcs]


def expected(R, per_doc, peers):
    """The restatement over every doc: (kinds, message per doc)."""
    kinds, msgs = [], []
    for d, sources in enumerate(per_doc):
        k, m = model.extract_doc_ref(sources, peers[d])
        kinds += k
        msgs.append(m)
    return np.array(kinds, dtype=np.uint8), msgs


def assert_message(got, kind, srcs, want_kinds, want_msgs, tombs=True):
    """got (host SrcBatch) bit-exact against the restatement's message; tombs False: the call
    passed no tombstone arrays (kind None: no kind array), the rest is checked as ever."""
    want = src_batch_of(srcs.R, want_msgs)
    ns = srcs.n_srcs
    if kind is not None:
        assert (kind == want_kinds).all(), np.nonzero(kind != want_kinds)[0][:8]
    assert (got.doc_srcs == srcs.doc_srcs).all()
    assert (got.src_actor[:ns] == srcs.src_actor[:ns]).all()
    assert (got.vv[: ns * srcs.R] == srcs.vv[: ns * srcs.R]).all()
    # the packed offsets are the running sums of what each source keeps
    assert (got.entry_off == want.entry_off).all(), "entry_off"
    if tombs:
        assert (got.tomb_off == want.tomb_off).all(), "tomb_off"
    te, tt = int(want.entry_off[ns]), int(want.tomb_off[ns])
    cols = (("keys", te), ("actors", te), ("counters", te), ("tkeys", tt), ("tactors", tt), ("tcounters", tt))
    for f, n in cols if tombs else cols[:3]:
        g, w = getattr(got, f)[:n], getattr(want, f)[:n]
        assert (g == w).all(), (f, np.nonzero(g != w)[0][:8])


def parity_case(R, n_docs, seed):
    """Sources per doc from {0, 1, 3, 10}; entries per source from {0, 1, 8, 63,
    64, 65, 130}, tombstones from {0, 1, 2, 64, 65}; actors up to R + 1 (never R).
    A tenth of the docs are quiet (every dot below R and covered by the peer, no
    tombstones), so that NONE occurs; zeros in the peer clock give FULL."""
    rng = random.Random(seed)
    per_doc, peers = [], []
    for _ in range(n_docs):
        quiet = rng.random() < 0.1
        sources = []
        for _ in range(rng.choice([0, 1, 3, 10])):
            ne = rng.choice([0, 1, 1, 8, 8, 8, 8, 63, 64, 65, 130])
            nt = 0 if quiet else rng.choice([0, 1, 1, 2, 2, 2, 64, 65])
            sources.append(model.random_source(rng, R, ne, nt, 400, 12, actor_hi=R - 1 if quiet else None))
        per_doc.append(sources)
        peers.append([12] * R if quiet else [rng.choice([0, rng.randint(1, 12)]) for _ in range(R)])
    return per_doc, peers


_cases = {}


def case(R):
    """(per_doc, peers, host SrcBatch, expected kinds, expected messages), made once per R."""
    if R not in _cases:
        per_doc, peers = parity_case(R, 3000, 1000 + R)
        kinds, msgs = expected(R, per_doc, peers)
        _cases[R] = (per_doc, peers, src_batch_of(R, per_doc), kinds, msgs)
    return _cases[R]


# ---------------------------------------------------------------- oracle parity

@pytest.mark.parametrize("R", [2, 16, 64])
def test_oracle_parity(eng, torch, R):
    per_doc, peers, srcs, kinds, msgs = case(R)
    assert {int(k) for k in kinds} == {NONE, DELTA, FULL}
    got, kind = extract(eng, torch, srcs, np.array(peers, dtype=U64).reshape(-1))
    assert_message(got, kind, srcs, kinds, msgs)


# ---------------------------------------------------------------- round trip through the fold

def test_round_trip_through_fold(eng, torch):
    """fold(DELTA, dst, extract(srcs, peer)) == fold(DELTA, dst, srcs), per doc,
    for peer = dst.vv and for a stale clock.  Doc 0: under the stale clock its
    second source is FULL (the peer never met actor 1), but the receiver has met
    it by then -- the first source raises its counter -- and takes the delta
    path, where the shipped tombstone removes key 7."""
    R = 16
    rng = random.Random(77)
    per_doc = [s for s in case(R)[0][:600]]
    dsts = [random_state(rng, R, rng.randint(0, 64), 400, 12, actor_hi=R + 1) for _ in per_doc]
    dsts = [([(k, a if a != R else 0, c) for k, a, c in e], vv) for e, vv in dsts]
    z = [0] * (R - 2)
    dsts[0] = ([(7, 0, 1), (9, 0, 2)], [2, 0] + z)
    per_doc[0] = [(0, [3, 2] + z, [(9, 0, 2), (11, 0, 3)], None),
                  (1, [3, 4] + z, [(12, 1, 4)], [(7, 1, 3)])]
    dst, srcs = batch_of(R, dsts), src_batch_of(R, per_doc)
    full = eng.fold(CRDT_FOLD_DELTA, dst, srcs)
    assert out_doc(full, 0, R)[0] == [(9, 0, 2), (11, 0, 3), (12, 1, 4)]
    exact = np.array(dst.vv, dtype=U64)
    stale = np.array([rng.randint(0, int(x)) for x in exact], dtype=U64)
    stale[: R] = [1, 0] + z
    for what, peer in (("exact", exact), ("stale", stale)):
        msg, kind = eng.delta_extract(srcs, peer)
        if what == "stale":
            assert list(kind[:2]) == [DELTA, FULL]
        assert int(msg.entry_off[-1]) < int(srcs.entry_off[-1])  # it ships less than the states
        got = eng.fold(CRDT_FOLD_DELTA, dst, msg)
        for d in range(dst.n_docs):
            assert out_doc(got, d, R) == out_doc(full, d, R), (what, d)


# ---------------------------------------------------------------- edges

def test_no_docs_and_no_sources(eng, torch):
    R = 4
    dev = torch.device("cuda:0")
    for n_docs in (0, 5):
        # all zeros: no doc has a source (room for one, so that every array has an address)
        srcs = SrcBuffers(R, n_docs, 1, 1, 1, device=dev)
        out = SrcBuffers(R, n_docs, 1, 1, 1, device=dev)
        for f in ("doc_srcs", "entry_off", "tomb_off"):
            getattr(out, f).fill_(-1)
        eng.delta_extract_async(srcs, to_dev(torch, np.zeros(n_docs * R, U64)), out)  # (kind may be NULL)
        eng.sync()
        torch.cuda.synchronize()
        got = out.numpy()
        assert (got.doc_srcs == 0).all() and len(got.doc_srcs) == n_docs + 1
        assert int(got.entry_off[0]) == 0 and int(got.tomb_off[0]) == 0


def test_without_tombstone_arrays(eng, torch):
    """srcs->tomb_off == NULL: no tombstones; the tomb_off the output passes is zeroed."""
    R = 3
    rng = random.Random(5)
    per_doc = [[model.random_source(rng, R, rng.choice([0, 3, 70]), 0, 200, 9) for _ in range(rng.randint(0, 4))]
               for _ in range(200)]
    peers = [[rng.choice([0, rng.randint(1, 9)]) for _ in range(R)] for _ in per_doc]
    srcs = src_batch_of(R, per_doc)
    kinds, msgs = expected(R, per_doc, peers)
    bare = SrcBatch(R, srcs.doc_srcs, srcs.src_actor, srcs.vv, srcs.entry_off, srcs.keys, srcs.actors, srcs.counters)
    dev = torch.device("cuda:0")
    out = SrcBuffers(R, srcs.n_docs, srcs.n_srcs, int(srcs.entry_off[-1]), 0, device=dev)
    out.tomb_off.fill_(-1)
    kind = torch.zeros(srcs.n_srcs, dtype=torch.uint8, device=dev)
    eng.delta_extract_async(bare.to(dev), to_dev(torch, np.array(peers, dtype=U64).reshape(-1)), out, kind=kind)
    eng.sync()
    torch.cuda.synchronize()
    assert_message(out.numpy(), kind.cpu().numpy(), srcs, kinds, msgs)
    assert (out.numpy().tomb_off == 0).all()


def test_one_large_source(eng, torch):
    """One doc, one source of 5,000 entries and 300 tombstones (chunks of 64, staged once)."""
    R = 16
    rng = random.Random(9)
    per_doc = [[model.random_source(rng, R, 5000, 300, 20000, 12)]]
    per_doc[0][0] = (3,) + per_doc[0][0][1:]
    srcs = src_batch_of(R, per_doc)
    for peer in ([5] * R, [0] * R):  # DELTA, then FULL
        kinds, msgs = expected(R, per_doc, [peer])
        got, kind = extract(eng, torch, srcs, np.array(peer, dtype=U64))
        assert_message(got, kind, srcs, kinds, msgs)
    assert 0 < int(got.tomb_off[-1]) < 300


@pytest.mark.parametrize("R,n_docs", [(64, 8191), (64, 8192), (64, 8193), (16, 4 * 8192 + 1)])
def test_scan_chunk_edges(eng, torch, R, n_docs):
    """One one-entry source per doc, n_docs around the scan's chunk of 8,192 groups
    of 64 / R docs; the expectation is the rule written with numpy."""
    rng = np.random.default_rng(n_docs + R)
    srcs = SrcBuffers(R, n_docs, n_docs, n_docs, 0)
    srcs.doc_srcs[:] = np.arange(n_docs + 1)
    srcs.entry_off[:] = np.arange(n_docs + 1)
    srcs.src_actor[:] = rng.integers(0, R, n_docs)
    srcs.vv[:] = rng.integers(0, 9, n_docs * R)
    srcs.keys[:] = rng.integers(0, 1 << 40, n_docs)
    srcs.actors[:] = rng.integers(0, R, n_docs)
    srcs.counters[:] = rng.integers(1, 6, n_docs)
    peer = rng.integers(0, 6, (n_docs, R)).astype(U64)
    full = peer[np.arange(n_docs), srcs.src_actor] == 0
    keep = full | (peer[np.arange(n_docs), srcs.actors] < srcs.counters)
    got, kind = extract(eng, torch, srcs, peer.reshape(-1))
    assert (kind == np.where(full, FULL, np.where(keep, DELTA, NONE))).all()
    assert (got.entry_off == np.concatenate([[0], np.cumsum(keep)])).all()
    assert (got.tomb_off == 0).all()
    n = int(keep.sum())
    for f in ("keys", "actors", "counters"):
        assert (getattr(got, f)[:n] == getattr(srcs, f)[keep]).all(), f
    assert (got.src_actor == srcs.src_actor).all() and (got.vv[: n_docs * R] == srcs.vv).all()
    assert (got.doc_srcs == srcs.doc_srcs).all()


# ---------------------------------------------------------------- panic parity

def test_panic_parity(torch):
    R = 4
    e = crdtgpu.Engine(0)
    try:
        ok = (0, [1] * R, [(3, 1, 1)], [(5, R, 1)])  # (a tombstone dot at actor == R is never tested)
        cases = [
            ([[ok], [(R, [1] * R, [], None)]], [[1] * R] * 2, True),   # Counter(src_actor == R)
            ([[ok], [(0, [1] * R, [(3, R, 1)], None)]], [[1] * R] * 2, True),   # HasDot on the DELTA path
            ([[ok], [(0, [1] * R, [(3, R, 1)], None)]], [[1] * R, [0] + [1] * (R - 1)], False),  # the same, FULL
        ]
        for per_doc, peers, panics in cases:
            srcs = src_batch_of(R, per_doc)
            if panics:
                with pytest.raises(ref.GoPanic):
                    expected(R, per_doc, peers)
                with pytest.raises(crdtgpu.CrdtError) as ei:
                    extract(e, torch, srcs, np.array(peers, dtype=U64).reshape(-1))
                assert ei.value.code == crdtgpu.CRDT_E_ACTOR_RANGE
            else:
                kinds, msgs = expected(R, per_doc, peers)
                assert list(kinds) == [DELTA, FULL]
                got, kind = extract(e, torch, srcs, np.array(peers, dtype=U64).reshape(-1))
                assert_message(got, kind, srcs, kinds, msgs)
        # a later clean call on the same engine succeeds
        per_doc, peers = [[ok]], [[1] * R]
        kinds, msgs = expected(R, per_doc, peers)
        srcs = src_batch_of(R, per_doc)
        got, kind = extract(e, torch, srcs, np.array(peers, dtype=U64).reshape(-1))
        assert_message(got, kind, srcs, kinds, msgs)
    finally:
        e.close()


# ---------------------------------------------------------------- host path

def test_host_path(eng, torch):
    R = 2
    per_doc, peers, srcs, kinds, msgs = case(R)
    per_doc, peers = per_doc[:500], peers[:500]
    srcs = src_batch_of(R, per_doc)
    kinds, msgs = expected(R, per_doc, peers)
    peer = np.array(peers, dtype=U64).reshape(-1)
    want, wkind = extract(eng, torch, srcs, peer)
    msg, kind = eng.delta_extract(srcs, peer)
    assert_message(msg, kind, srcs, kinds, msgs)
    assert (kind == wkind).all() and kind.dtype == np.uint8
    te, tt = int(want.entry_off[-1]), int(want.tomb_off[-1])
    assert len(msg.keys) == te and len(msg.tkeys) == tt  # trimmed to the packed sizes
    for f in ("doc_srcs", "src_actor", "entry_off", "tomb_off"):
        assert (getattr(msg, f) == getattr(want, f)).all(), f
    for f, n in (("keys", te), ("actors", te), ("counters", te), ("tkeys", tt), ("tactors", tt), ("tcounters", tt)):
        assert (getattr(msg, f) == getattr(want, f)[:n]).all(), f


@pytest.mark.parametrize("where", ["entries", "tombstones"])
def test_host_path_rejects_unsorted_keys(eng, where):
    R = 2
    good = (0, [1, 1], [(1, 0, 1), (4, 1, 2)], [(2, 0, 1), (6, 0, 1)])
    bad = (0, [1, 1], [(4, 0, 1), (1, 1, 2)], []) if where == "entries" else (0, [1, 1], [], [(6, 0, 1), (2, 0, 1)])
    with pytest.raises(crdtgpu.CrdtError) as ei:
        eng.delta_extract(src_batch_of(R, [[good], [good, bad]]), np.ones(2 * R, U64))
    assert ei.value.code == crdtgpu.CRDT_E_UNSORTED
    msg, kind = eng.delta_extract(src_batch_of(R, [[good]]), np.ones(R, U64))  # the engine is usable afterwards
    assert list(kind) == [DELTA] and int(msg.entry_off[-1]) == 1 and int(msg.tomb_off[-1]) == 2


# ---------------------------------------------------------------- graph capture

def test_graph_capture(torch):
    """Without crdt_ctx_reserve a call inside a capture that would have to grow the
    workspace returns CRDT_E_WORKSPACE; after reserve it captures, and the replay
    is bit-exact."""
    R = 16
    per_doc, peers, _, _, _ = case(R)
    per_doc, peers = per_doc[:2000], peers[:2000]
    srcs = src_batch_of(R, per_doc)
    kinds, msgs = expected(R, per_doc, peers)
    e = crdtgpu.Engine(0)
    try:
        ds, out, kind = device_buffers(torch, srcs)
        dp = to_dev(torch, np.array(peers, dtype=U64).reshape(-1))
        small = src_batch_of(R, per_doc[:8])
        s_ds, s_out, s_kind = device_buffers(torch, small)
        e.delta_extract_async(s_ds, dp, s_out, kind=s_kind, stream=torch.cuda.current_stream())  # eager, 8 docs
        e.sync(torch.cuda.current_stream())
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.delta_extract_async(ds, dp, out, kind=kind, stream=torch.cuda.current_stream())
        assert ei.value.code == crdtgpu.CRDT_E_WORKSPACE
        e.reserve(srcs.n_docs)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.delta_extract_async(ds, dp, out, kind=kind, stream=torch.cuda.current_stream())
        for _ in range(2):
            for f, _dt in SrcBatch._FIELDS:
                getattr(out, f).fill_(-1)
            kind.fill_(77)
            g.replay()
            e.sync(torch.cuda.current_stream())
            torch.cuda.synchronize()
            assert_message(out.numpy(), kind.cpu().numpy()[: srcs.n_srcs], srcs, kinds, msgs)
    finally:
        e.close()
