"""GPU: apply_kernel (csrc/apply.hip) on every case of tests/apply_edge_cases.py (pinned
by tests/test_apply_edges_model.py), bit-exact against the map-based replay and the C
oracle.

Every output array is pre-filled with a pattern no case holds, and the whole arrays are
compared with an image built from the expected documents: offsets, counts and clocks,
the live prefix of every document, and the pattern in every slot outside a live prefix.
A refused document must come out with count 0 (include/crdtgpu.h: offsets and counts are
written for every doc); only its own slots and clock are left out of the comparison.  No test provokes a fault: the error cases are the reported ones of the
contract (the head of csrc/apply.hip).
"""

import numpy as np
import pytest

import crdtgpu
from apply_cases import doc_of, tomb_batch
from apply_edge_cases import (ADD, CASES, DDEL, DDK, DEL, Case, Doc, R, batches, doc, ents_of, expected, expected_doc,
                              mixed_doc, op_batch, state_batch)
from crdtgpu import CRDT_E_ACTOR_RANGE, CRDT_E_CAPACITY, CRDT_E_INVALID
from crdtgpu.batch import OpBatch, OutBuffers, TombBuffers
from oracle import oracle
from test_gpu_compare import _code, dev_of

pytestmark = pytest.mark.gpu

U8, U32, U64 = np.uint8, np.uint32, np.uint64
P32, P64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A  # no case holds these as a key, an actor, a counter or a clock
OUT_F = ("offsets", "counts", "keys", "actors", "counters", "vv")
TOMB_F = ("offsets", "counts", "keys", "actors", "counters")


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

def slots_of(x):
    return int(np.asarray(x.offsets)[-1]) if x is not None else 0


def poison(torch, buf, fields):
    for f in fields:
        t = getattr(buf, f)
        t.fill_(P32 if t.dtype == torch.int32 else P64)
    return buf


def slots_of_ops(op):
    return int(np.asarray(op.op_off)[-1])


def poisoned(torch, st, tb, op, tombs_out=True):
    """Poisoned (OutBuffers, TombBuffers or None) of exactly the capacity the call needs."""
    n, nops = st.n_docs, slots_of_ops(op)
    out = poison(torch, OutBuffers(n, R, slots_of(st) + nops, device=dev_of(torch)), OUT_F)
    tout = poison(torch, TombBuffers(n, slots_of(tb) + nops, device=dev_of(torch)), TOMB_F) if tombs_out else None
    return out, tout


def download(buf, fields):
    got = {}
    for f in fields:
        a = getattr(buf, f).cpu().numpy()
        got[f] = a.view(U32 if a.dtype == np.int32 else U64)
    return got


class Image:
    """The arrays a call must leave behind: the expected documents at their offsets, the
    poison everywhere else; a refused document has count 0, and `care` is False over its slots
    and its clock, which are undefined."""

    def __init__(self, st, tb, op, want, refused=(), tombs_out=True):
        n, nops = st.n_docs, slots_of_ops(op)
        op_off = np.asarray(op.op_off).astype(np.int64)
        self.n = n
        self.parts = []
        lists = [(np.asarray(st.offsets).astype(np.int64) + op_off, slots_of(st) + nops, 0, True)]
        if tombs_out:
            toff = np.asarray(tb.offsets).astype(np.int64) if tb is not None else np.zeros(n + 1, np.int64)
            lists.append((toff + op_off, slots_of(tb) + nops, 1, False))
        for off, slots, which, with_vv in lists:
            img = dict(offsets=off.astype(U32), counts=np.full(n, P32, U32), keys=np.full(slots, P64, U64),
                       actors=np.full(slots, P32, U32), counters=np.full(slots, P64, U64))
            care = {f: np.ones(len(a), bool) for f, a in img.items()}
            if with_vv:
                img["vv"] = np.full(n * R, P64, U64)
                care["vv"] = np.ones(n * R, bool)
            for d, w in enumerate(want):
                lo, hi = int(off[d]), int(off[d + 1])
                if d in refused:
                    img["counts"][d] = 0  # written for every document: a refused one comes out empty
                    for f in ("keys", "actors", "counters"):
                        care[f][lo:hi] = False
                    if with_vv:
                        care["vv"][d * R:(d + 1) * R] = False
                    continue
                rows = w[which]
                assert lo + len(rows) <= hi
                img["counts"][d] = len(rows)
                if rows:
                    k, a, c = zip(*rows)
                    img["keys"][lo:lo + len(rows)] = np.array(k, U64)
                    img["actors"][lo:lo + len(rows)] = np.array(a, U32)
                    img["counters"][lo:lo + len(rows)] = np.array(c, U64)
                if with_vv:
                    img["vv"][d * R:(d + 1) * R] = np.array(w[2], U64)
            self.parts.append((img, care))

    def check(self, out, tout, what=""):
        for (img, care), buf, fields, name in zip(self.parts, (out, tout), (OUT_F, TOMB_F), ("entries", "tombstones")):
            got = download(buf, fields)
            for f, a in img.items():
                g = got[f][: len(a)]
                bad = np.flatnonzero((g != a) & care[f])
                assert bad.size == 0, "%s %s.%s[%d] = %#x, want %#x" % (what, name, f, bad[0], int(g[bad[0]]),
                                                                         int(a[bad[0]]))


def run_async(eng, torch, st, tb, op, tombs_out=True, stream=None):
    dev = dev_of(torch)
    out, tout = poisoned(torch, st, tb, op, tombs_out)
    eng.apply_async(st.to(dev), op.to(dev), out, tb.to(dev) if tb is not None else None, tout, stream=stream)
    return out, tout


def oracle_docs(st, tb, op, with_tombs=True):
    rc, wo, wt = oracle.apply(st, op, tb, with_tombs=with_tombs)
    assert rc == 0
    return [doc_of(wo, wt, d, R) for d in range(st.n_docs)]


# ------------------------------------------------------------- 1. the case table

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_into_poisoned_buffers(eng, torch, case):
    st, tb, op = batches(case)
    want = expected(case)
    assert oracle_docs(st, tb, op) == want
    out, tout = run_async(eng, torch, st, tb, op)
    eng.sync()
    Image(st, tb, op, want).check(out, tout, case.name)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_case_on_the_host_path(eng, case):
    st, tb, op = batches(case)
    want = expected(case)
    go, gt = eng.apply(st, op, tb)
    op_off = np.asarray(op.op_off)
    assert (go.offsets == np.asarray(st.offsets) + op_off).all()
    assert (gt.offsets == (np.asarray(tb.offsets) if tb is not None else 0) + op_off).all()
    assert go.counts.tolist() == [len(w[0]) for w in want] and gt.counts.tolist() == [len(w[1]) for w in want]
    assert go.vv.tolist() == [x for w in want for x in w[2]]
    for d, w in enumerate(want):
        assert doc_of(go, gt, d, R) == w, (case.name, d)


# ------------------------------------- 2. a refused document among good ones

def long_doc(i, ddk=True):
    """A neighbour: 256 ops; ddk False: ADD and DEL only."""
    if ddk:
        return mixed_doc(256, actor=i % R, shift=i)
    u = 90
    ops = [((ADD, DEL, ADD)[(i + j) % 3], 10 * ((j * 7 + i) % u + 1)) for j in range(256)]
    return doc(ops, ents_of([10 * (j + 1) for j in range(0, u, 2)]), ents_of([15, 25], actor=2), actor=i % R)


SOME = ents_of([20, 30, 40])
REFUSALS = {
    # name: (the refused document, the code crdt_ctx_sync returns, tomb_out given)
    "257_ops": (doc([(ADD, 3 * j + 1) for j in range(257)], SOME, ents_of([5])), CRDT_E_INVALID, True),
    "kind_4": (doc([(ADD, 15), (4, 20), (DEL, 30)], SOME, ents_of([5])), CRDT_E_INVALID, True),
    "ddk_first": (doc([(DDK, 20), (ADD, 15)], SOME, ents_of([5])), CRDT_E_INVALID, True),
    "ddk_after_add": (doc([(DDEL, 0), (ADD, 15), (DDK, 20)], SOME, ents_of([5])), CRDT_E_INVALID, True),
    "bump_with_actor_R": (doc([(DEL, 20), (ADD, 15)], SOME, ents_of([5]), actor=R), CRDT_E_ACTOR_RANGE, True),
    "ddk_without_tomb_out": (doc([(DDEL, 0), (DDK, 20)], SOME, ents_of([5])), CRDT_E_INVALID, False),
}


@pytest.mark.parametrize("kind", list(REFUSALS))
def test_refused_document_among_good_ones(eng, torch, kind):
    bad, code, tombs_out = REFUSALS[kind]
    for pos in (0, 2, 4):
        docs = [long_doc(i, ddk=tombs_out) for i in range(5)]
        docs[pos] = bad
        st, tb, op = state_batch(docs), tomb_batch([d.tombs for d in docs]), op_batch(docs)
        want = [None if d == pos else expected_doc(x) for d, x in enumerate(docs)]
        out, tout = run_async(eng, torch, st, tb, op, tombs_out)
        assert _code(eng.sync) == code, (kind, pos)
        eng.sync()  # cleared
        # the offsets of every document (the refused one's too), every other document exact
        Image(st, tb, op, want, refused={pos}, tombs_out=tombs_out).check(out, tout, "%s at %d" % (kind, pos))
    # the engine is usable afterwards
    good = Case("after", [long_doc(1), long_doc(2)], {})
    st, tb, op = batches(good)
    out, tout = run_async(eng, torch, st, tb, op)
    eng.sync()
    Image(st, tb, op, expected(good)).check(out, tout, "after " + kind)


# ------------------------------------------------ 3. grid stride and stale LDS

def stride_batch(n):
    """n tiny documents (at most 4 entries and 4 ops); every third is a 256-op run on one
    key; every seventh is refused, by each refusal kind in turn.  Returns the batches, the
    op batch with the refused scripts emptied, and the refused ids."""
    docs, refused = [], set()
    runs = ([((DEL, ADD)[j % 2], 70) for j in range(256)], [((ADD, DEL)[j % 2], 70) for j in range(256)])
    bad = [REFUSALS[k][0].ops for k in ("kind_4", "ddk_first", "ddk_after_add", "bump_with_actor_R", "257_ops")]
    tiny = ([(ADD, 15), (DEL, 30)], [(DDEL, 0), (DDK, 20), (DDK, 25), (ADD, 20)], [], [(DEL, 70), (ADD, 90), (DDEL, 0)],
            [(ADD, 70)])
    for d in range(n):
        ents = ents_of([10 * (j + 2) + (d % 2) * 40 for j in range(d % 5)])
        tombs = ents_of([10 * (j + 1) + 5 for j in range(d % 3)], actor=2)
        if d % 7 == 3:
            refused.add(d)
            k = (d // 7) % len(bad)
            docs.append(Doc(R if k == 3 else d % R, ents, tombs, [d % 11, 3, d % 5], bad[k]))
        elif d % 3 == 0:
            docs.append(Doc(d % R, ents, tombs, [d % 11, 3, d % 5], runs[d % 2]))
        else:
            docs.append(Doc(d % R, ents, tombs, [d % 11, 3, d % 5], tiny[d % len(tiny)]))
    st, tb = state_batch(docs), tomb_batch([d.tombs for d in docs])
    return st, tb, packed_ops(docs), packed_ops(docs, without=refused), refused


def packed_ops(docs, without=()):
    """op_batch for many documents that share a few scripts: each script is packed once."""
    arrays = {}
    for x in docs:
        if id(x.ops) not in arrays:
            arrays[id(x.ops)] = (np.array([k for k, _ in x.ops], U8), np.array([v for _, v in x.ops], U64))
    none = (np.zeros(0, U8), np.zeros(0, U64))
    per = [none if d in without else arrays[id(x.ops)] for d, x in enumerate(docs)]
    op_off = np.zeros(len(docs) + 1, U32)
    np.cumsum([len(p[0]) for p in per], out=op_off[1:])
    return OpBatch(op_off, np.concatenate([p[0] for p in per] + [np.zeros(1, U8)]),
                   np.concatenate([p[1] for p in per] + [np.zeros(1, U64)]), np.array([x.actor for x in docs], U32))


def test_grid_stride_and_stale_lds(eng, torch):
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2 * (2 * 16 * cus) + 3  # the grid is 16 workgroups of 2 waves per CU: every wave takes 2 documents, some 3
    st, tb, op, emptied, refused = stride_batch(n)
    assert len(refused) > n // 8 and max(int(x) for x in np.diff(op.op_off)) == 257
    want = oracle_docs(st, tb, emptied)
    out, tout = run_async(eng, torch, st, tb, op)
    assert _code(eng.sync) == CRDT_E_ACTOR_RANGE  # reported before CRDT_E_INVALID (crdt_ctx_sync)
    eng.sync()
    Image(st, tb, op, want, refused=refused).check(out, tout, "stride")


# ------------------------------------------------------ 4. tomb_out == NULL

def test_null_tomb_out_leaves_deleted_alone(eng, torch):
    """tombs given, live tombstones in every document, ADD and DEL only, tomb_out NULL: no
    tombstone is read or written; entries and clocks are the oracle's."""
    docs = [long_doc(i, ddk=False) for i in range(3)] + [doc([(ADD, 15), (DEL, 20)], SOME, ents_of(range(5, 700, 10)))]
    assert all(d.tombs for d in docs)
    st, tb, op = state_batch(docs, 2), tomb_batch([d.tombs for d in docs], 2), op_batch(docs)
    want = oracle_docs(st, tb, op, with_tombs=False)
    assert [w[:1] + w[2:] for w in want] == [(e, vv) for e, _, vv in map(expected_doc, docs)]
    dev = dev_of(torch)
    dtb = tb.to(dev)
    out, _ = poisoned(torch, st, tb, op, tombs_out=False)
    eng.apply_async(st.to(dev), op.to(dev), out, dtb, None)
    eng.sync()
    Image(st, tb, op, want, tombs_out=False).check(out, None, "tomb_out NULL")
    for f in TOMB_F:  # the input tombstones, slack included, are as they were
        assert (download(dtb, (f,))[f] == np.asarray(getattr(tb, f))).all(), f
    go, gt = eng.apply(st, op, tb, with_tombs=False)
    assert gt is None
    for d, w in enumerate(want):
        assert doc_of(go, None, d, R) == w, d


# ------------------------------------------------------ 5. count above slots

@pytest.mark.parametrize("which", ["state", "tombs"])
def test_count_above_slots_is_clamped(eng, torch, which):
    docs = [mixed_doc(12 + 5 * i, actor=i % R, shift=i) for i in range(5)]
    st, tb, op = state_batch(docs, 1), tomb_batch([d.tombs for d in docs], 1), op_batch(docs)
    x = st if which == "state" else tb
    # the middle document's one slack slot holds a well-formed row above its live keys, so the
    # clamped document is pinned too: exactly its slots, that row included, and no more
    last = int(x.offsets[3]) - 1
    extra = (10 ** 6, 1, 7)
    x.keys[last], x.actors[last], x.counters[last] = extra
    x.counts[2] = int(x.offsets[3]) - int(x.offsets[2]) + 9
    out, tout = run_async(eng, torch, st, tb, op)
    assert _code(eng.sync) == CRDT_E_CAPACITY
    eng.sync()  # cleared
    field = "ents" if which == "state" else "tombs"
    full = docs[2]._replace(**{field: getattr(docs[2], field) + [extra]})
    want = [expected_doc(full if d == 2 else v) for d, v in enumerate(docs)]
    x.counts[2] = int(x.offsets[3]) - int(x.offsets[2])  # the oracle on the count the clamp gives
    assert oracle_docs(st, tb, op) == want
    Image(st, tb, op, want).check(out, tout, which)


# -------------------------------------------------------------- 6. graph capture

def test_graph_capture(torch):
    """One stream: apply_async captured, replayed, the op keys changed in place, replayed
    again; both results exact."""
    docs = [c.docs[0] for c in CASES if not c.null_tombs and not c.slack][::3] + [mixed_doc(256), mixed_doc(255, 1, 1)]
    moved = [d._replace(ops=[(kind, k if kind == DDEL else (k + 10) % (1 << 64)) for kind, k in d.ops]) for d in docs]
    st, tb, op = state_batch(docs), tomb_batch([d.tombs for d in docs]), op_batch(docs)
    op2 = op_batch(moved)
    assert (op2.kind == op.kind).all() and (op2.keys != op.keys).any()
    dev = dev_of(torch)
    e = crdtgpu.Engine(0)
    try:
        e.reserve(st.n_docs)
        dst, dtb, dop = st.to(dev), tb.to(dev), op.to(dev)
        out, tout = poisoned(torch, st, tb, op)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.apply_async(dst, dop, out, dtb, tout, stream=torch.cuda.current_stream())
        for hop, hdocs in ((op, docs), (op2, moved)):
            dop.keys.copy_(hop.to(dev).keys)
            poison(torch, out, OUT_F)
            poison(torch, tout, TOMB_F)
            g.replay()
            e.sync(torch.cuda.current_stream())
            Image(st, tb, hop, [expected_doc(d) for d in hdocs]).check(out, tout, "replay")
    finally:
        e.close()
