"""GPU: crdt_awset_sources_async (csrc/sources.hip) against sources_ref
(tests/sources_cases.py, pinned by tests/test_sources_model.py), bit-exact.

Every output buffer is pre-filled with poison (words all-ones), so each word read
back was written by the call, and entry and tombstone slots at or past the
totals must still hold it.  The kernels work in these units, and the edge cases
below are sized around them:
  kSrcScanChunk   = 1,024 sources per workgroup of the offset scan (count per
                    chunk, scan of the partials, emit),
  kSrcPartStep    = 1,024 partial sums per step of the one-workgroup partials
                    scan (more than 1,024 x 1,024 sources: it steps),
  kSrcGatherChunk = 2,048 output positions per gather step,
  kSrcRun         = 1,024 sources of a gather chunk staged in LDS at most.
"""

import ctypes
import random

import numpy as np
import pytest

import crdtgpu
import test_delta_extract_model as model
from apply_cases import make_case
from crdtgpu import CRDT_FOLD_AWSET, CRDT_FOLD_DELTA, abi
from crdtgpu.batch import AWSetBatch, OutBuffers, Replica, SrcBatch, SrcBuffers, TombBatch, TombBuffers
from helpers import batch_of, out_doc, src_batch_of
from oracle import oracle
from sources_cases import (K_GATHER, K_PART, K_RUN, K_SCAN, MAXK, ONES32, U32, make_replica,
                           rand_docs, rand_replicas, sources_ref, tiny_replicas)
from test_gpu_compare import _code, dev_of, host_out

pytestmark = pytest.mark.gpu

ENTRY = ("keys", "actors", "counters")
TOMB = ("tkeys", "tactors", "tcounters")


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

def poison(out):
    for f, _ in SrcBatch._FIELDS:
        t = getattr(out, f)
        if t is not None:
            t.fill_(-1)


def poisoned_src(torch, R, n_docs, n_srcs, e_slots, t_slots, tombs="all"):
    """Device output buffers filled with all-ones words.  tombs: "all", "off" (only
    tomb_off is passed) or "none" (NULL tombstone arrays)."""
    out = SrcBuffers(R, n_docs, n_srcs, e_slots, t_slots, device=dev_of(torch))
    if tombs != "all":
        out.tkeys = out.tactors = out.tcounters = None
    if tombs == "none":
        out.tomb_off = None
    poison(out)
    out.e_slots, out.t_slots = e_slots, t_slots
    return out


def assert_sources(out, ref):
    """A poisoned device output equals ref (SourcesRef): every word of doc_srcs,
    src_actor, vv, entry_off and tomb_off, the entries and tombstones below the
    totals written, every slot at or past them still poison."""
    h, w = out.numpy(), ref.msg
    ns, R = w.n_srcs, w.R
    assert (h.doc_srcs == w.doc_srcs).all(), "doc_srcs"
    assert (h.src_actor[:ns] == w.src_actor).all(), "src_actor"
    assert (h.vv[: ns * R] == w.vv).all(), "vv"
    assert (h.entry_off == w.entry_off).all(), "entry_off"
    if h.tomb_off is not None:
        assert (h.tomb_off == w.tomb_off).all(), "tomb_off"
    for fields, n, slots in ((ENTRY, ref.n_e, out.e_slots), (TOMB, ref.n_t, out.t_slots)):
        for f in fields:
            g = getattr(h, f)
            if g is None:
                assert n == 0
                continue
            x = getattr(w, f)[:n]
            if not (g[:n] == x).all():
                i = int(np.nonzero(g[:n] != x)[0][0])
                raise AssertionError("%s differs first at %d of %d: gpu %d, expected %d" % (f, i, n, g[i], x[i]))
            assert (g[n:slots] == (ONES32 if g.dtype == U32 else MAXK)).all(), f + " written at or past the total"
    return h


def sources_on_device(eng, torch, reps, spare=3, entry_slots=None, tomb_slots=None, tombs="all", dev_reps=None,
                      ref=None, stream=None):
    """(poisoned output after one call, ref); the call is not synced."""
    ref = ref or sources_ref(reps, entry_slots, tomb_slots)
    te, tt = int(ref.msg.entry_off[-1]), int(ref.msg.tomb_off[-1])
    s0 = reps[0].state
    out = poisoned_src(torch, s0.R, s0.n_docs, s0.n_docs * len(reps), te + spare, tt + spare, tombs)
    dev = dev_of(torch)
    eng.sources_async(dev_reps or [r.to(dev) for r in reps], out,
                      entry_slots=te + spare if entry_slots is None else entry_slots,
                      tomb_slots=tt + spare if tomb_slots is None else tomb_slots, stream=stream)
    return out, ref


def check_sources(eng, torch, reps, **kw):
    out, ref = sources_on_device(eng, torch, reps, **kw)
    eng.sync()
    assert not ref.capacity
    assert_sources(out, ref)
    return ref


def host_state(out):
    """A device join / apply output as the host batch it is, as it stands."""
    h = host_out(out)
    return AWSetBatch(out.R, h.offsets, h.keys, h.actors, h.counters, h.vv, counts=h.counts)


def seq_list(start, n, R=2):
    return [(start + 2 * i, i % R, 7 * i + 1) for i in range(n)]


# ------------------------------------------------------------ 1. random small

@pytest.mark.parametrize("R", [1, 3, 64])
@pytest.mark.parametrize("P", [1, 2, 3, 16])
def test_random_small(eng, torch, P, R):
    """2,000 documents, replicas in mixed layouts (rand_replicas: slack 0 and 3,
    counts given and NULL, stale slack, empty documents, documents of tombstones
    only, replica 1 without tombstones, scalar and per-document actors); replica 0's
    state is a join output used as it stands (capacity offsets, counts, padded slack)."""
    n = 2000
    dev = dev_of(torch)
    reps_docs, reps = rand_replicas(8000 + 17 * P + R, n, P, R, max_e=12 if P < 16 else 5, max_t=4 if P < 16 else 2)
    other = make_replica(R, rand_docs(random.Random(8100 + P + R), R, n, max_e=6), tombs=False).state
    a = reps[0].state
    jo = OutBuffers(n, R, int(a.offsets[-1]) + int(other.offsets[-1]), device=dev)
    for t in (jo.keys, jo.actors, jo.counters):
        t.fill_(-1)  # what the join does not write is never read
    eng.join_async(a.to(dev), other.to(dev), jo)
    eng.sync()
    joined = host_state(jo)
    assert (np.diff(joined.offsets.astype(np.int64)) > joined.counts).any()  # capacity offsets: slack after the live prefix
    reps[0] = Replica(joined, reps[0].tombs, reps[0].actor, reps[0].doc_actor)
    dev_reps = [r.to(dev) for r in reps]
    dev_reps[0] = Replica(jo.as_batch(), dev_reps[0].tombs, reps[0].actor, dev_reps[0].doc_actor)
    ref = check_sources(eng, torch, reps, dev_reps=dev_reps)
    assert int(ref.msg.entry_off[-1]) > n and int(ref.msg.tomb_off[-1]) > n // 4
    cnt = np.diff(ref.msg.entry_off.astype(np.int64)) + np.diff(ref.msg.tomb_off.astype(np.int64))
    assert (cnt == 0).any()  # sources with nothing to copy


# ---------------------------------------------------------- 2. scan edges

@pytest.mark.parametrize("P,n_docs", [(1, K_SCAN - 1), (1, K_SCAN), (1, K_SCAN + 1), (3, 341), (3, 342),
                                      (2, K_SCAN), (16, 3 * K_SCAN // 16 + 1)])
def test_scan_chunk_edges(eng, torch, P, n_docs):
    reps = tiny_replicas(8200 + n_docs + P, n_docs, P, R=2)
    check_sources(eng, torch, reps)


_big = {}


def big_case():
    """2^20 + 1 sources (P = 1) of 0 to 2 entries and 0 or 1 tombstones: 1,025 scan
    chunks, so the partials scan steps; the expectation is the vectorised reference."""
    if not _big:
        reps = tiny_replicas(8300, K_PART * K_SCAN + 1, 1)
        _big.update(reps=reps, ref=sources_ref(reps))
    return _big["reps"], _big["ref"]


def test_partials_scan_steps(eng, torch):
    reps, ref = big_case()
    assert (ref.msg.n_srcs + K_SCAN - 1) // K_SCAN == K_PART + 1
    out, _ = sources_on_device(eng, torch, reps, ref=ref)
    eng.sync()
    assert_sources(out, ref)


# -------------------------------------------------------- 3. gather edges

_edge = {}


def edge_case():
    """Two replicas whose OUTPUT has: documents of 2,047, 1, 2,048, 2,049 and 4,097
    entries of replica 0, each followed by a 0- to 3-entry document of replica 1
    (so later runs start at odd positions and pairs straddle sources); 1,500
    documents of 0 or 1 entries on both sides (3,000 sources in under 2,048
    positions: more than kSrcRun, the unstaged search); then 300 documents of odd
    sizes.  The tombstones have the same sizes."""
    if not _edge:
        rng = random.Random(8400)
        sizes0 = [2047, 1, 2048, 2049, 4097] + [i % 2 for i in range(1500)] + [rng.choice((1, 3, 5)) for _ in range(300)]
        sizes1 = [rng.randint(0, 3) for _ in range(5)] + [(i // 2) % 2 for i in range(1500)] + \
                 [rng.choice((1, 2, 3)) for _ in range(300)]
        docs = [[], []]
        for p, sizes in enumerate((sizes0, sizes1)):
            for d, m in enumerate(sizes):
                docs[p].append((seq_list(10 * d + p, m), seq_list(10 * d + p + 5, m), [d + 1, p + 3]))
        _edge.update(docs=docs)
    return _edge["docs"]


@pytest.mark.parametrize("slack0,slack1", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gather_chunk_edges(eng, torch, slack0, slack1):
    """Slack 0: runs start where the last ended and pairs at even source slots are read
    with 16 B loads; slack 1: source runs start at odd slots on that replica."""
    docs = edge_case()
    reps = [make_replica(2, docs[0], slack=slack0, with_counts=True, garbage=np.random.default_rng(1), actor=0),
            make_replica(2, docs[1], slack=slack1, with_counts=True, garbage=np.random.default_rng(2), actor=1)]
    ref = check_sources(eng, torch, reps)
    eo = ref.msg.entry_off.astype(np.int64)
    assert (np.diff(eo)[[0, 2, 4, 6, 8]] == [2047, 1, 2048, 2049, 4097]).all()
    per_chunk = np.bincount(np.minimum(eo[:-1] // K_GATHER, eo[-1] // K_GATHER))
    assert per_chunk.max() > K_RUN  # some gather chunk holds more sources than are staged
    assert (eo[:-1][np.diff(eo) > 1] % 2 == 1).any()  # runs that start at odd output positions
    assert (ref.msg.tomb_off == ref.msg.entry_off).all()


def shifted(torch, t):
    """The same values in a tensor whose first element sits one element past an aligned address."""
    big = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    big[1:].copy_(t)
    return big[1:]


@pytest.mark.parametrize("where", ["sources", "output", "both"])
def test_unaligned_columns_give_the_same_result(eng, torch, where):
    """Column pointers one element off 16 B: the gather goes element by element on
    that side, and the result is identical to the aligned run."""
    docs = edge_case()
    dev = dev_of(torch)
    reps = [make_replica(2, docs[0], actor=0), make_replica(2, docs[1], slack=1, actor=1)]
    ref = sources_ref(reps)
    dev_reps = [r.to(dev) for r in reps]
    if where != "output":
        r = dev_reps[1]
        for cols in (r.state, r.tombs):
            for f in ("keys", "actors", "counters"):
                setattr(cols, f, shifted(torch, getattr(cols, f)))
                assert getattr(cols, f).data_ptr() % (8 if f == "actors" else 16) != 0
    te, tt = ref.n_e, ref.n_t
    out = poisoned_src(torch, 2, reps[0].n_docs, 2 * reps[0].n_docs, te + 3, tt + 3)
    if where != "sources":
        for f in ENTRY + TOMB:
            setattr(out, f, shifted(torch, getattr(out, f)))
            assert getattr(out, f).data_ptr() % 16 != 0
    eng.sources_async(dev_reps, out, entry_slots=te + 3, tomb_slots=tt + 3)
    eng.sync()
    assert_sources(out, ref)


# ------------------------------------------------------------------ 4. clocks

@pytest.mark.parametrize("R", [1, 3, 64])
def test_clock_widths_and_actors(eng, torch, R):
    _, reps = rand_replicas(8500 + R, 300, 3, R)
    ref = check_sources(eng, torch, reps)
    n, P = 300, 3
    assert (ref.msg.vv.reshape(n, P, R)[7, 2] == reps[2].state.vv.reshape(n, R)[7]).all()
    assert (ref.msg.src_actor.reshape(n, P)[:, 1] == reps[1].doc_actor).all()
    assert (ref.msg.src_actor.reshape(n, P)[:, 2] == reps[2].actor).all()


# --------------------------------------------------------- 5. tombstone forms

@pytest.mark.parametrize("tombs", ["none", "off"])
def test_no_replica_has_tombstones(eng, torch, tombs):
    """NULL tombstone arrays in out; a tomb_off that out does pass comes out zeroed."""
    rng = random.Random(8600)
    reps = [make_replica(3, rand_docs(rng, 3, 1500), slack=p, tombs=False, actor=p) for p in range(2)]
    out, ref = sources_on_device(eng, torch, reps, tombs=tombs)
    eng.sync()
    h = assert_sources(out, ref)
    assert ref.n_t == 0
    if tombs == "off":
        assert (h.tomb_off == 0).all() and len(h.tomb_off) == 3001


def test_some_replicas_have_tombstones(eng, torch):
    rng = random.Random(8601)
    reps = [make_replica(2, rand_docs(rng, 2, 1200), slack=p % 2, tombs=p in (1, 3), actor=p % 2) for p in range(4)]
    ref = check_sources(eng, torch, reps)
    t = np.diff(ref.msg.tomb_off.astype(np.int64)).reshape(1200, 4)
    assert not t[:, 0].any() and not t[:, 2].any() and t[:, 1].any() and t[:, 3].any()


# ------------------------------------------------------------------ 6. errors

@pytest.mark.parametrize("which", ["entries", "tombstones"])
def test_count_above_slots_is_clamped(eng, torch, which):
    rng = random.Random(8700)
    reps = [make_replica(2, rand_docs(rng, 2, 40, max_e=5, max_t=2), slack=1, garbage=np.random.default_rng(3)),
            make_replica(2, rand_docs(rng, 2, 40, max_e=5, max_t=2), actor=1)]
    cols = reps[0].state if which == "entries" else reps[0].tombs
    cols.counts[9] = int(cols.offsets[10]) - int(cols.offsets[9]) + 5
    out, ref = sources_on_device(eng, torch, reps)
    assert ref.capacity
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    assert_sources(out, ref)
    eng.sync()  # cleared, and the engine is usable afterwards
    cols.counts[9] = 0
    check_sources(eng, torch, reps)


@pytest.mark.parametrize("which", ["entries", "tombstones"])
def test_total_one_above_the_slots(eng, torch, which):
    _, reps = rand_replicas(8701, 1500, 2, 2)
    full = sources_ref(reps)
    te, tt = int(full.msg.entry_off[-1]), int(full.msg.tomb_off[-1])
    es, ts = (te - 1, tt) if which == "entries" else (te, tt - 1)
    ref = sources_ref(reps, entry_slots=es, tomb_slots=ts)
    assert ref.capacity and (ref.n_e, ref.n_t) == (es, ts)
    out, _ = sources_on_device(eng, torch, reps, spare=3, entry_slots=es, tomb_slots=ts, ref=ref)
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    assert_sources(out, ref)  # offsets whole, poison intact at and past the slot limit
    eng.sync()


def test_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched."""
    dev = dev_of(torch)
    rng = random.Random(8702)
    reps = [make_replica(2, rand_docs(rng, 2, 6), slack=1, actor=p, doc_actor=[p] * 6).to(dev) for p in range(2)]
    bare = make_replica(2, rand_docs(rng, 2, 6), tombs=False).to(dev)
    r3 = make_replica(3, rand_docs(rng, 3, 6)).to(dev)
    n7 = make_replica(2, rand_docs(rng, 2, 7)).to(dev)
    out = poisoned_src(torch, 2, 6, 12, 200, 200)
    lib, ctx, INV = abi.lib(), eng._ctx, crdtgpu.CRDT_E_INVALID

    def call(rs, co, n=None):
        cr = [r.c() if hasattr(r, "c") else r for r in rs]
        arr = (abi.CReplica * max(len(cr), 1))(*cr)
        return lib.crdt_awset_sources_async(ctx, arr, len(cr) if n is None else n, 200, 200,
                                            ctypes.byref(co) if co is not None else None, None)

    assert call(reps, out.c_delta_out()) == 0
    eng.sync()
    poison(out)
    assert call(reps, out.c_delta_out(), n=0) == INV
    assert call(reps * 9, out.c_delta_out()) == INV  # 18 replicas
    assert lib.crdt_awset_sources_async(ctx, None, 2, 200, 200, ctypes.byref(out.c_delta_out()), None) == INV
    assert call(reps, None) == INV
    no_state = reps[1].c()
    no_state.state = None
    assert call([reps[0], no_state], out.c_delta_out()) == INV
    for f in ("doc_srcs", "src_actor", "vv", "entry_off", "keys", "actors", "counters",
              "tomb_off", "tkeys", "tactors", "tcounters"):  # the tombstone arrays: a replica has tombstones
        co = out.c_delta_out()
        setattr(co, f, None)
        assert call(reps, co) == INV, f
    assert call([reps[0], n7], out.c_delta_out()) == INV  # n_docs
    assert call([reps[0], r3], out.c_delta_out()) == INV  # R
    for bad_r in (0, 65):
        cs = [r.c() for r in reps]
        keep = []
        for c in cs:
            st = reps[0].state.c()
            st.R = bad_r
            keep.append(st)
            c.state = ctypes.addressof(st)
        assert call(cs, out.c_delta_out()) == INV, bad_r
    cs, keep = [r.c() for r in reps * 8], []
    for c, r in zip(cs, reps * 8):  # 16 replicas of 2^28 documents: 2^32 sources
        st = r.state.c()
        st.n_docs = 1 << 28
        keep.append(st)
        c.state = ctypes.addressof(st)
    assert call(cs, out.c_delta_out()) == INV
    # an out array starting where the same-kind array of any replica starts
    for r in reps:
        pairs = [("entry_off", r.state.offsets), ("keys", r.state.keys), ("actors", r.state.actors),
                 ("counters", r.state.counters), ("vv", r.state.vv), ("src_actor", r.doc_actor),
                 ("tomb_off", r.tombs.offsets), ("tkeys", r.tombs.keys), ("tactors", r.tombs.actors),
                 ("tcounters", r.tombs.counters)]
        for f, t in pairs:
            co = out.c_delta_out()
            setattr(co, f, t.data_ptr())
            assert call(reps, co) == INV, f
    eng.sync()
    h = out.numpy()
    for f, _ in SrcBatch._FIELDS:
        g = getattr(h, f)
        assert (g == (ONES32 if g.dtype == U32 else MAXK)).all(), f
    # without tombstones anywhere the tombstone arrays are not required
    co = poisoned_src(torch, 2, 6, 6, 100, 0, tombs="none")
    assert call([bare], co.c_delta_out()) == 0
    eng.sync()
    assert_sources(co, sources_ref([bare.numpy()]))


def test_no_documents(eng, torch):
    dev = dev_of(torch)
    z = lambda dt: torch.zeros(1, dtype=dt, device=dev)  # noqa: E731
    e = AWSetBatch(2, z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64))
    t = TombBatch(z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64))
    assert e.n_docs == 0
    out = poisoned_src(torch, 2, 0, 1, 4, 4)
    eng.sources_async([Replica(e, t, actor=1), Replica(e)], out, entry_slots=4, tomb_slots=4)
    eng.sync()
    h = out.numpy()
    assert h.doc_srcs.tolist() == [0] and h.entry_off.tolist() == [0, ONES32] and h.tomb_off.tolist() == [0, ONES32]
    assert (h.keys == MAXK).all() and (h.tkeys == MAXK).all() and (h.vv == MAXK).all() and (h.src_actor == ONES32).all()


# ----------------------------------------------- 7. round trips on the device

def test_delta_round_on_the_device(eng, torch):
    """apply -> sources -> extract -> fold with nothing downloaded in between: Add and
    AWSetDelta.Del op lists applied to two resident AWSetDelta replicas, each apply
    output fed as it stands to sources_async, the delta extracted against the peer's
    clock and folded into the peer; against the same round through host-built
    source batches, the extraction's restatement and the C oracle's fold."""
    dev = dev_of(torch)
    R, n = 4, 600
    rng = random.Random(8800)
    sides = []
    for _ in range(2):
        st, tb, ops, want = make_case(rng, n, R, lambda: rng.randint(0, 12), lambda: rng.randint(0, 10), universe=60)
        assert all(w is not None for w in want)
        nops = int(ops.op_off[-1])
        out = OutBuffers(n, R, int(st.offsets[-1]) + nops, device=dev)
        tout = TombBuffers(n, int(tb.offsets[-1]) + nops, device=dev)
        dops = ops.to(dev)
        eng.apply_async(st.to(dev), dops, out, tb.to(dev), tout)
        sides.append(dict(out=out, tout=tout, ops=ops, dops=dops, want=want))
    got = []
    for me, peer in ((0, 1), (1, 0)):
        a, b = sides[me], sides[peer]
        e_slots, t_slots = a["out"].slots, int(a["tout"].keys.shape[0])
        srcs = poisoned_src(torch, R, n, n, e_slots, t_slots)
        msg = poisoned_src(torch, R, n, n, e_slots, t_slots)
        eng.sources_async([Replica(a["out"].as_batch(), a["tout"], doc_actor=a["dops"].doc_actor)], srcs)
        eng.delta_extract_async(srcs, b["out"].vv, msg)
        res = OutBuffers(n, R, b["out"].slots + e_slots, device=dev)
        eng.reserve(n, res.slots)
        eng.fold_async(CRDT_FOLD_DELTA, b["out"].as_batch(), msg, res)
        got.append((srcs, res))
    eng.sync()
    for (me, peer), (srcs, res) in zip(((0, 1), (1, 0)), got):
        a, b = sides[me], sides[peer]
        actors = a["ops"].doc_actor
        per_doc = [[(int(actors[d]), w[2], w[0], w[1])] for d, w in enumerate(a["want"])]
        built = src_batch_of(R, per_doc)
        h = srcs.numpy()
        te, tt = int(built.entry_off[-1]), int(built.tomb_off[-1])
        assert (h.entry_off == built.entry_off).all() and (h.tomb_off == built.tomb_off).all() and tt > 0
        assert (h.keys[:te] == built.keys[:te]).all() and (h.tcounters[:tt] == built.tcounters[:tt]).all()
        msgs = [model.extract_doc_ref(per_doc[d], b["want"][d][2])[1] for d in range(n)]
        dst = batch_of(R, [(w[0], w[2]) for w in b["want"]])
        rc, want = oracle.fold(CRDT_FOLD_DELTA, dst, src_batch_of(R, msgs))
        assert rc == 0
        hr = host_out(res)
        changed = 0
        for d in range(n):
            assert out_doc(hr, d, R) == out_doc(want, d, R), (me, d)
            changed += out_doc(want, d, R) != dst.doc(d)
        assert changed > n // 2


def test_awset_fold_of_resident_replicas(eng, torch):
    """The two outputs of one exchange and a third state, as they stand, folded into a
    fourth with CRDT_FOLD_AWSET: r0 <- x_ab <- x_ba <- c."""
    dev = dev_of(torch)
    R, n = 3, 800
    rng = random.Random(8801)
    docs = [rand_docs(rng, R, n, max_e=10, max_t=0) for _ in range(4)]
    a, b, c, dst = (make_replica(R, dd, slack=s, tombs=False).state for dd, s in zip(docs, (0, 1, 3, 0)))
    slots = int(a.offsets[-1]) + int(b.offsets[-1])
    xab, xba = OutBuffers(n, R, slots, device=dev), OutBuffers(n, R, slots, device=dev)
    eng.exchange_async(a.to(dev), b.to(dev), xab, xba)
    reps = [Replica(xab.as_batch(), actor=0), Replica(xba.as_batch(), actor=1), Replica(c.to(dev), actor=2)]
    rc1, oab = oracle.join(a, b)
    rc2, oba = oracle.join(b, a)
    assert rc1 == 0 and rc2 == 0
    e_slots = int(oab.counts.sum()) + int(oba.counts.sum()) + c.live_slots()
    srcs = poisoned_src(torch, R, n, 3 * n, e_slots, 0, tombs="none")
    eng.sources_async(reps, srcs)
    res = OutBuffers(n, R, int(dst.offsets[-1]) + e_slots, device=dev)
    eng.reserve(n, res.slots)
    eng.fold_async(CRDT_FOLD_AWSET, dst.to(dev), srcs, res)
    eng.sync()
    per_doc = []
    for d in range(n):
        per_doc.append([(0,) + out_doc(oab, d, R)[::-1] + (None,), (1,) + out_doc(oba, d, R)[::-1] + (None,),
                        (2, docs[2][d][2], docs[2][d][0], None)])
    built = src_batch_of(R, per_doc)
    assert (srcs.numpy().entry_off == built.entry_off).all()
    rc, want = oracle.fold(CRDT_FOLD_AWSET, dst, built)
    assert rc == 0
    hr = host_out(res)
    for d in range(n):
        assert out_doc(hr, d, R) == out_doc(want, d, R), d


# -------------------------------------------------- 8. capture and determinism

def test_graph_capture(torch):
    """Captured on a reserved context and replayed twice, the output is identical each
    time and identical to the eager run; on a context whose workspace is too small
    for n_srcs the capture is refused with CRDT_E_WORKSPACE and launches nothing."""
    dev = dev_of(torch)
    _, reps = rand_replicas(8900, 1800, 3, 2)
    ref = sources_ref(reps)
    big, big_ref = big_case()
    assert (big_ref.msg.n_srcs + K_SCAN - 1) // K_SCAN > 1024  # (a fresh context's workspace holds 1,024 words)
    e = crdtgpu.Engine(0)
    try:
        dev_big = [r.to(dev) for r in big]
        out_big = poisoned_src(torch, 1, big[0].n_docs, big[0].n_docs, big_ref.n_e + 1, big_ref.n_t + 1)
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.sources_async(dev_big, out_big, stream=torch.cuda.current_stream())
        assert ei.value.code == crdtgpu.CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        h = out_big.numpy()
        assert (h.entry_off == ONES32).all() and (h.doc_srcs == ONES32).all() and (h.keys == MAXK).all()
        del dev_big, out_big
        e.reserve(ref.msg.n_srcs)
        dev_reps = [r.to(dev) for r in reps]
        out = poisoned_src(torch, 2, 1800, 5400, ref.n_e + 3, ref.n_t + 3)
        e.sources_async(dev_reps, out, stream=torch.cuda.current_stream())
        e.sync(torch.cuda.current_stream())
        eager = assert_sources(out, ref)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.sources_async(dev_reps, out, stream=torch.cuda.current_stream())
        for _ in range(2):
            poison(out)
            g.replay()
            e.sync(torch.cuda.current_stream())
            h = assert_sources(out, ref)
            for f, _dt in SrcBatch._FIELDS:
                assert (getattr(h, f) == getattr(eager, f)).all(), f
    finally:
        e.close()
