"""GPU: batched membership reads (crdt_awset_has_async / _batch,
crdt_tomb_has_async) against has_ref (tests/test_has_model.py), bit-exact.

Every output buffer is pre-filled with poison (found 77, dots all-ones), so
each word read back was written by the call.  The lookup kernel (csrc/query.hip)
takes chunks of kHasChunk = 256 threads x 4 queries = 1,024 consecutive queries
per workgroup, and stages the documents of a chunk in LDS when they are at most
kHasRun = 256 (otherwise lanes search q_off in global memory); the chunk-edge
cases below are sized around those two constants.
"""

import ctypes
import json
import random

import numpy as np
import pytest

import crdtgpu
from apply_cases import make_case
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch, OutBuffers, QueryBatch, QueryBuffers, TombBuffers
from helpers import GOLDEN, batch_of, random_state, snap_entries
from oracle import oracle
from test_has_model import has_ref

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
MAXK = 2 ** 64 - 1
K_HAS_CHUNK = 1024


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


def poisoned(torch, n_queries, dots=True):
    out = QueryBuffers(n_queries, device=torch.device("cuda:0"), dots=dots)
    out.found.fill_(77)
    if dots:
        out.actors.fill_(-1)
        out.counters.fill_(-1)
    return out


def assert_exact(got, want, dots=True):
    names = ("found", "actors", "counters") if dots else ("found",)
    for name, g, w in zip(names, got, want):
        assert g.shape == w.shape, name
        if not (g == w).all():
            i = int(np.nonzero(g != w)[0][0])
            raise AssertionError("%s differs first at query %d: gpu %d, expected %d" % (name, i, g[i], w[i]))


def has_on_device(eng, torch, state, per_doc, dots=True, stream=None, engine_call=None):
    """has_async of a host or device state for per-doc key lists -> numpy outputs."""
    dev = torch.device("cuda:0")
    q = QueryBatch.from_lists(per_doc)
    out = poisoned(torch, q.n_queries, dots)
    (engine_call or eng.has_async)(state.to(dev), q.to(dev), out, stream=stream)
    eng.sync(stream)
    return out.numpy()


# ------------------------------------------------------------------ 1. golden

def test_golden_states(eng, torch):
    g = json.load(open(GOLDEN))
    n = 0
    for sc in g["scenarios"]:
        snaps = list(sc["final"].values())
        for m in sc["merges"]:
            snaps += [m["dst"], m["src"], m["out"]]
        universe = sorted({e[0] for s in snaps for e in s["entries"] + s.get("deleted", [])})
        ids = {k: i for i, k in enumerate(universe)}
        R = max(len(s["vv"]) for s in snaps)
        b = batch_of(R, [(snap_entries(s, ids), s["vv"] + [0] * (R - len(s["vv"]))) for s in snaps])
        per_doc = [list(range(len(universe))) + [len(universe) + 5] for _ in snaps]
        assert_exact(has_on_device(eng, torch, b, per_doc), has_ref(b, per_doc))
        n += len(snaps)
    assert n >= 23 * 3


# ------------------------------------------------------------ 2. random small

LIVE = (0, 1, 2, 63, 64, 65, 200)
QUERIES = (0, 0, 1, 5, 64, 300)
_small = {}


def small_case(slack, with_counts, n_docs=2000):
    """(batch, per-doc queries, has_ref of them), built once per layout."""
    key = (slack, with_counts)
    if key in _small:
        return _small[key]
    rng = random.Random(7000 + 10 * slack + with_counts)
    R = 2
    doc_keys, stale = [], []
    for _ in range(n_docs):
        n = rng.choice(LIVE)
        ks = set()
        if n and rng.random() < 0.3:
            ks.add(0)
        if n > 1 and rng.random() < 0.3:
            ks.add(MAXK)
        while len(ks) < n:
            ks.add(rng.getrandbits(64))
        doc_keys.append(sorted(ks))
        stale.append(rng.choice(doc_keys[-1]) if n and rng.random() < 0.5 else rng.getrandbits(64))
    counts = np.array([len(k) for k in doc_keys], U32)
    offsets = np.zeros(n_docs + 1, U32)
    np.cumsum(counts + U32(slack), out=offsets[1:])
    total = int(offsets[-1])
    keys, actors, counters = np.zeros(total, U64), np.zeros(total, U32), np.zeros(total, U64)
    for d, ks in enumerate(doc_keys):
        o, n = int(offsets[d]), len(ks)
        keys[o:o + n] = ks
        actors[o:o + n] = [rng.randrange(R + 1) for _ in ks]
        counters[o:o + n] = [rng.randint(1, 2 ** 40) for _ in ks]
        if slack:  # slack holds keys that are queried: 0, 2^64-1 and a stale or random one
            keys[o + n:o + n + slack] = [0, MAXK, stale[d]][:slack]
            actors[o + n:o + n + slack] = 9
            counters[o + n:o + n + slack] = 99
    b = AWSetBatch(R, offsets, keys, actors, counters, np.zeros(n_docs * R, U64),
                   counts=counts if (slack or with_counts) else None)
    per_doc = []
    for d, ks in enumerate(doc_keys):
        qs = []
        for _ in range(rng.choice(QUERIES)):
            kind = rng.randrange(7)
            if kind == 0 and ks:
                qs.append(rng.choice(ks))
            elif kind == 1 and len(ks) > 1:
                j = rng.randrange(len(ks) - 1)
                qs.append(rng.randint(ks[j], ks[j + 1]) if ks[j + 1] - ks[j] > 1 else ks[j])
            elif kind == 2 and ks and ks[0] > 0:
                qs.append(rng.randrange(ks[0]))
            elif kind == 3 and ks and ks[-1] < MAXK:
                qs.append(rng.randint(ks[-1] + 1, MAXK))
            elif kind == 4:
                qs.append(0)
            elif kind == 5:
                qs.append(MAXK)
            else:
                qs.append(stale[d])
        per_doc.append(qs)
    _small[key] = (b, per_doc, has_ref(b, per_doc))
    return _small[key]


LAYOUTS = [(0, 0), (0, 1), (3, 1)]  # (slack, counts given); counts == NULL only at zero slack


@pytest.mark.parametrize("slack,with_counts", LAYOUTS)
def test_random_small(eng, torch, slack, with_counts):
    b, per_doc, want = small_case(slack, with_counts)
    assert (b.counts is None) == (not slack and not with_counts)
    assert 0 < want[0].sum() < len(want[0])
    assert_exact(has_on_device(eng, torch, b, per_doc), want)


# -------------------------------------------------- 3. a merge output as state

_join = {}


def join_case():
    if not _join:
        rng = random.Random(7100)
        R, n, universe = 3, 600, 50
        dst = batch_of(R, [random_state(rng, R, rng.randint(0, 40), universe, 30) for _ in range(n)])
        src = batch_of(R, [random_state(rng, R, rng.randint(0, 40), universe, 30) for _ in range(n)])
        rc, want_out = oracle.join(dst, src)
        assert rc == 0
        per_doc = [[0] + [rng.randrange(universe + 2) for _ in range(rng.randint(0, 30))] for _ in range(n)]
        want = has_ref(want_out.as_batch(), per_doc)
        first = np.cumsum([0] + [len(q) for q in per_doc[:-1]])  # the key-0 query of each doc
        assert 0 < want[0][first].sum() < n  # key 0 live in some documents, not in others
        _join.update(R=R, n=n, dst=dst, src=src, per_doc=per_doc, want=want)
    return _join


def test_join_output_is_a_state(eng, torch):
    """The join's crdt_awset_out (capacity offsets, zero-padded slack) queried as
    it stands, with no host round trip between the two calls."""
    c = join_case()
    dev = torch.device("cuda:0")
    out = OutBuffers(c["n"], c["R"], int(c["dst"].offsets[-1]) + int(c["src"].offsets[-1]), device=dev)
    q = QueryBatch.from_lists(c["per_doc"])
    res = poisoned(torch, q.n_queries)
    eng.join_async(c["dst"].to(dev), c["src"].to(dev), out)
    eng.has_async(out.as_batch(), q.to(dev), res)
    eng.sync()
    assert_exact(res.numpy(), c["want"])


# ------------------------------------------------------------- 4. chunk edges

def _tiny_state(n_docs):
    """n_docs documents of two live keys 10 d + 1 and 10 d + 5, one slack slot holding 10 d + 7."""
    d = np.arange(n_docs, dtype=U64)
    keys = np.stack([10 * d + 1, 10 * d + 5, 10 * d + 7], axis=1).reshape(-1)
    offsets = (3 * np.arange(n_docs + 1)).astype(U32)
    return AWSetBatch(2, offsets, keys, (np.arange(3 * n_docs) % 3).astype(U32),
                      np.arange(1, 3 * n_docs + 1, dtype=U64), np.zeros(2 * n_docs, U64),
                      counts=np.full(n_docs, 2, U32))


def _tiny_queries(rng, d, n):
    return [10 * d + rng.choice([0, 1, 3, 5, 7, 9]) for _ in range(n)]


@pytest.mark.parametrize("total", [K_HAS_CHUNK - 1, K_HAS_CHUNK, K_HAS_CHUNK + 1, 2 * K_HAS_CHUNK + 1])
def test_chunk_edge_totals(eng, torch, total):
    rng = random.Random(7200 + total)
    n_docs = 37
    cuts = sorted(rng.randint(0, total) for _ in range(n_docs - 1))
    sizes = [b - a for a, b in zip([0] + cuts, cuts + [total])]
    b = _tiny_state(n_docs)
    per_doc = [_tiny_queries(rng, d, n) for d, n in enumerate(sizes)]
    assert sum(len(q) for q in per_doc) == total
    assert_exact(has_on_device(eng, torch, b, per_doc), has_ref(b, per_doc))


def test_one_document_spans_several_workgroups(eng, torch):
    rng = random.Random(7201)
    b = _tiny_state(3)
    per_doc = [_tiny_queries(rng, 0, 3), _tiny_queries(rng, 1, 3 * K_HAS_CHUNK + 5), _tiny_queries(rng, 2, 3)]
    assert_exact(has_on_device(eng, torch, b, per_doc), has_ref(b, per_doc))


def test_long_run_of_documents_without_queries(eng, torch):
    """One query, 100,000 documents that ask nothing, one query, ten documents
    of one query: the 12 queries share a chunk whose documents span far more
    than the staged run, so lanes search q_off in global memory (the staged arm
    is what every other case here takes)."""
    rng = random.Random(7202)
    n_docs = 1 + 100000 + 1 + 10
    b = _tiny_state(n_docs)
    per_doc = [[] for _ in range(n_docs)]
    for d in [0] + list(range(100001, n_docs)):
        per_doc[d] = [10 * d + rng.choice([1, 5])] if d % 3 else [10 * d + rng.choice([0, 7])]
    want = has_ref(b, per_doc)
    assert 0 < want[0].sum() < 12
    assert_exact(has_on_device(eng, torch, b, per_doc), want)
    # the same layout twice over: a chunk whose span is wide, then a narrow one
    per_doc2 = [list(q) for q in per_doc]
    per_doc2[n_docs - 1] = _tiny_queries(rng, n_docs - 1, 2 * K_HAS_CHUNK)
    assert_exact(has_on_device(eng, torch, b, per_doc2), has_ref(b, per_doc2))


# ----------------------------------------------------------- 5. large document

def test_large_document(eng, torch):
    rng = random.Random(7300)
    n = (1 << 20) + 1
    big = 3 * np.arange(n, dtype=U64) + 1
    keys = np.concatenate([big, np.array([12345], U64)])
    b = AWSetBatch(2, np.array([0, n, n + 1, n + 1], U32), keys, (np.arange(n + 1) % 5).astype(U32),
                   np.arange(n + 1, dtype=U64) + 2 ** 33, np.zeros(6, U64))
    q0 = []
    for i in (0, n - 1, n // 2, 1, n - 2):
        k = 3 * i + 1
        q0 += [k, k - 1, k + 1]
    q0 += [0, MAXK, 3 * n + 1]
    while len(q0) < 4096:
        q0.append(rng.randrange(3 * n + 5))
    rng.shuffle(q0)
    per_doc = [q0, [12345, 12344], [0, 1, MAXK]]
    want = has_ref(b, per_doc)
    assert want[0][:4096].sum() > 1000 and want[0][-3:].sum() == 0
    assert_exact(has_on_device(eng, torch, b, per_doc), want)


# --------------------------------------------------------- 6. optional outputs

def test_found_alone(eng, torch):
    b, per_doc, want = small_case(3, 1)
    got = has_on_device(eng, torch, b, per_doc, dots=False)
    assert got[1] is None and got[2] is None
    assert_exact(got, want, dots=False)


# ---------------------------------------------------------------- 7. tombstones

def test_tombstones_of_an_apply_run(eng, torch):
    rng = random.Random(7400)
    R, n, universe = 4, 800, 120
    st, tb, op, want_docs = make_case(rng, n, R, lambda: rng.randint(0, 60), lambda: rng.randint(0, 30),
                                      universe=universe)
    assert any(w[1] for w in want_docs)
    dev = torch.device("cuda:0")
    nops = int(op.op_off[-1])
    out = OutBuffers(n, R, int(st.offsets[-1]) + nops, device=dev)
    tout = TombBuffers(n, int(tb.offsets[-1]) + nops, device=dev)
    per_doc = [[t[0] for t in w[1]] + [rng.randrange(universe + 3) for _ in range(rng.randint(0, 12))]
               for w in want_docs]
    q = QueryBatch.from_lists(per_doc)
    res = poisoned(torch, q.n_queries)
    eng.apply_async(st.to(dev), op.to(dev), out, tb.to(dev), tout)
    eng.tomb_has_async(tout, q.to(dev), res)
    eng.sync()
    found, actors, counters = [], [], []
    for w, qs in zip(want_docs, per_doc):
        deleted = {k: (a, c) for k, a, c in w[1]}  # the reference's Deleted after the ops
        for k in qs:
            a, c = deleted.get(k, (0, 0))
            found.append(k in deleted)
            actors.append(a)
            counters.append(c)
    assert_exact(res.numpy(), (np.array(found, U8), np.array(actors, U32), np.array(counters, U64)))


# -------------------------------------------------------------------- 8. errors

def test_async_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched."""
    dev = torch.device("cuda:0")
    b = batch_of(2, [([(1, 0, 1), (4, 1, 2)], [1, 2]), ([(3, 0, 1)], [1, 0])]).to(dev)
    q = QueryBatch.from_lists([[1, 2], [3]]).to(dev)
    out = poisoned(torch, 3)
    lib, ctx = abi.lib(), eng._ctx
    ref = ctypes.byref

    def call(cb, cq, co):
        return lib.crdt_awset_has_async(ctx, ref(cb) if cb else None, ref(cq) if cq else None,
                                        ref(co) if co else None, None)

    assert call(None, q.c(), out.c()) == crdtgpu.CRDT_E_INVALID
    assert call(b.c(), None, out.c()) == crdtgpu.CRDT_E_INVALID
    assert call(b.c(), q.c(), None) == crdtgpu.CRDT_E_INVALID
    cq = q.c()
    cq.q_off = None
    assert call(b.c(), cq, out.c()) == crdtgpu.CRDT_E_INVALID
    cq = q.c()
    cq.keys = None
    assert call(b.c(), cq, out.c()) == crdtgpu.CRDT_E_INVALID
    cq = q.c()
    cq.n_docs = 3
    assert call(b.c(), cq, out.c()) == crdtgpu.CRDT_E_INVALID
    for field in ("found", "actors", "counters"):
        co = out.c()
        setattr(co, field, None)
        assert call(b.c(), q.c(), co) == crdtgpu.CRDT_E_INVALID, field
    cb = b.c()
    cb.R = 65
    assert call(cb, q.c(), out.c()) == crdtgpu.CRDT_E_INVALID
    # the tombstone form: the same checks, n_docs passed beside the view
    tb = TombBuffers(2, 4, device=dev)
    tb.offsets.zero_()
    tb.counts.zero_()
    ct = tb.c()
    assert lib.crdt_tomb_has_async(ctx, None, 2, ref(q.c()), ref(out.c()), None) == crdtgpu.CRDT_E_INVALID
    assert lib.crdt_tomb_has_async(ctx, ref(ct), 3, ref(q.c()), ref(out.c()), None) == crdtgpu.CRDT_E_INVALID
    eng.sync()
    got = out.numpy()
    assert (got[0] == 77).all() and (got[1] == 2 ** 32 - 1).all() and (got[2] == MAXK).all()  # nothing ran
    # n_queries == 0: CRDT_OK, nothing launched, outputs untouched
    q0 = QueryBatch.from_lists([[], []]).to(dev)
    eng.has_async(b, q0, out)
    eng.tomb_has_async(tb, q0, out)
    eng.sync()
    got = out.numpy()
    assert (got[0] == 77).all() and (got[1] == 2 ** 32 - 1).all() and (got[2] == MAXK).all()
    # and the call still works
    eng.has_async(b, q, out)
    eng.sync()
    assert_exact(out.numpy(), (np.array([1, 0, 1], U8), np.array([0, 0, 0], U32), np.array([1, 0, 1], U64)))


def test_host_form_errors(eng):
    good = batch_of(2, [([(1, 0, 1), (4, 1, 2)], [1, 2]), ([(3, 0, 1)], [1, 0]), ([], [0, 0])])
    keys = np.array([1, 2, 3, 4], U64)

    def code(state, q):
        with pytest.raises(crdtgpu.CrdtError) as ei:
            eng.has(state, q)
        return ei.value.code

    assert code(good, QueryBatch(np.array([0, 3, 2, 4], U32), keys, 4)) == crdtgpu.CRDT_E_INVALID  # not monotone
    assert code(good, QueryBatch(np.array([1, 2, 3, 4], U32), keys, 4)) == crdtgpu.CRDT_E_INVALID  # q_off[0] != 0
    assert code(good, QueryBatch(np.array([0, 1, 2, 3], U32), keys, 4)) == crdtgpu.CRDT_E_INVALID  # != n_queries
    assert code(good, QueryBatch(np.array([0, 2, 4], U32), keys, 4)) == crdtgpu.CRDT_E_INVALID  # n_docs mismatch
    q = QueryBatch.from_lists([[1, 2], [3], [4]])
    unsorted = batch_of(2, [([(4, 0, 1), (1, 1, 2)], [1, 2]), ([(3, 0, 1)], [1, 0]), ([], [0, 0])])
    assert code(unsorted, q) == crdtgpu.CRDT_E_UNSORTED
    over = batch_of(2, [([(1, 0, 1)], [1, 0]), ([(3, 0, 1)], [1, 0]), ([], [0, 0])], slack=1)
    over.counts[1] = 5
    assert code(over, q) == crdtgpu.CRDT_E_CAPACITY
    found, actors, counters = eng.has(good, QueryBatch.from_lists([[], [], []]))  # n_queries == 0
    assert len(found) == len(actors) == len(counters) == 0
    found, actors, counters = eng.has(good, q)  # the context is still usable
    assert found.tolist() == [1, 0, 1, 0] and actors.tolist() == [0, 0, 0, 0] and counters.tolist() == [1, 0, 1, 0]


# ---------------------------------------------------------- 9. streams, capture

def test_ordered_after_a_join_on_another_stream(eng, torch):
    c = join_case()
    dev = torch.device("cuda:0")
    out = OutBuffers(c["n"], c["R"], int(c["dst"].offsets[-1]) + int(c["src"].offsets[-1]), device=dev)
    for t in (out.offsets, out.counts, out.keys, out.actors, out.counters, out.vv):
        t.zero_()  # a lookup that ran before the join would find nothing
    dd, ds = c["dst"].to(dev), c["src"].to(dev)
    q = QueryBatch.from_lists(c["per_doc"]).to(dev)
    res = poisoned(torch, q.n_queries)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.join_async(dd, ds, out, stream=sa)
    eng.has_async(out.as_batch(), q, res, stream=sb)
    eng.sync(sb)
    assert_exact(res.numpy(), c["want"])


def test_captured_on_an_unreserved_context(eng, torch):
    b, per_doc, want = small_case(3, 1)
    dev = torch.device("cuda:0")
    bd, q = b.to(dev), QueryBatch.from_lists(per_doc).to(dev)
    eager = poisoned(torch, q.n_queries)
    eng.has_async(bd, q, eager)
    eng.sync()
    assert_exact(eager.numpy(), want)
    e = crdtgpu.Engine(0)  # fresh: nothing reserved, no call made on it yet
    try:
        res = poisoned(torch, q.n_queries)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.has_async(bd, q, res, stream=torch.cuda.current_stream())
        for _ in range(2):
            res.found.fill_(77)
            res.actors.fill_(-1)
            res.counters.fill_(-1)
            g.replay()
            e.sync(torch.cuda.current_stream())
            assert_exact(res.numpy(), eager.numpy())
    finally:
        e.close()


# ------------------------------------------------------------------ 10. host form

@pytest.mark.parametrize("slack,with_counts", LAYOUTS)
def test_host_form_equals_async(eng, torch, slack, with_counts):
    b, per_doc, want = small_case(slack, with_counts)
    got = eng.has(b, QueryBatch.from_lists(per_doc))
    assert_exact(got, has_on_device(eng, torch, b, per_doc))
    assert_exact(got, want)
