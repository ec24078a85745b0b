"""GPU: the scatter (crdt_awset_scatter_async) against scatter_ref
(tests/test_scatter_model.py), bit-exact.

Every output buffer is pre-filled with poison (words all-ones), so each word
read back was written by the call, and entry slots at or past offsets[n_docs]
must still hold it.  The kernels (csrc/scatter.hip) work in these units, and the
edge cases below are sized around them:
  kSctScanChunk   = 1,024 documents per workgroup of the offset scan (count per
                    chunk, scan of the partials, emit),
  kSctPartStep    = 1,024 partial sums per step of the one-workgroup partials
                    scan (more than 1,024 x 1,024 documents: it steps),
  kSctGatherChunk = 2,048 output positions per gather step,
  kSctRun         = 1,024 documents of a gather chunk staged in LDS at most.
"""

import ctypes
import random

import numpy as np
import pytest

import crdtgpu
from crdtgpu import abi
from crdtgpu.batch import AWSetBatch, OutBuffers
from helpers import batch_of
from oracle import oracle
from test_compare_model import KEYS, compare_ref, select_ref
from test_gpu_compare import (_code, _rand_doc, _seq_doc, assert_cmp, assert_packed, dev_of, host_out, pack,
                              poisoned_cmp, poisoned_out, read_cmp, xchg_case)
from test_scatter_model import one_entry_case, scatter_ref

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
MAXK = 2 ** 64 - 1
ONES32 = 2 ** 32 - 1
K_SCAN = 1024     # kSctScanChunk
K_PART = 1024     # kSctPartStep
K_GATHER = 2048   # kSctGatherChunk
K_RUN = 1024      # kSctRun


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


def dev_words(torch, words):
    a = np.ascontiguousarray(np.asarray(words, dtype=U32))
    if a.size == 0:
        a = np.zeros(1, U32)
    return torch.from_numpy(a.view(np.int32)).to(dev_of(torch))


def scatter_on_device(eng, torch, state, sub, idx, n_idx=None, spare=3, out_slots=None, total=None, stream=None):
    """The poisoned output of one scatter of host batches, after the sync."""
    dev = dev_of(torch)
    if total is None:
        total = int(scatter_ref(state, sub, idx, n_idx).offsets[-1])
    out = poisoned_out(torch, state.n_docs, state.R, total + spare)
    eng.scatter_async(state.to(dev), sub.to(dev), dev_words(torch, idx), out,
                      n_idx=None if n_idx is None else dev_words(torch, [n_idx]), out_slots=out_slots, stream=stream)
    return out


def check_scatter(eng, torch, state, sub, idx, n_idx=None):
    want = scatter_ref(state, sub, idx, n_idx)
    out = scatter_on_device(eng, torch, state, sub, idx, n_idx, total=int(want.offsets[-1]))
    eng.sync()
    assert_packed(out, want)
    return want


# ------------------------------------------------------------ 1. random small

LAYOUTS = [(0, 0), (0, 1), (3, 1)]  # (slack, counts given); counts == NULL only at zero slack
_small = {}


def small_docs(n_docs=2000, n_sub=700):
    """State documents of 0 to 40 entries and, for a random subset in random
    order, replacements that are longer, shorter, empty or of the same length."""
    if not _small:
        rng = random.Random(9800)
        R = 2
        st = [_rand_doc(rng, R, rng.randint(0, 40)) for _ in range(n_docs)]
        idx = rng.sample(range(n_docs), n_sub)
        sub, seen = [], {"longer": 0, "shorter": 0, "empty": 0, "same": 0, "was_empty": 0}
        for j, d in enumerate(idx):
            n = len(st[d][0])
            kind = ("longer", "shorter", "empty", "same")[j % 4]
            if kind == "shorter" and n == 0:
                kind = "longer"
            m = {"longer": n + rng.randint(1, 10), "shorter": rng.randint(0, max(n - 1, 0)), "empty": 0, "same": n}[kind]
            sub.append(_rand_doc(rng, R, m))
            seen[kind] += 1
            seen["was_empty"] += n == 0 and m > 0
        _small.update(R=R, st=st, sub=sub, idx=np.array(idx, U32), seen=seen)
    return _small


@pytest.mark.parametrize("sub_slack,sub_counts", LAYOUTS)
@pytest.mark.parametrize("st_slack,st_counts", LAYOUTS)
def test_random_small(eng, torch, st_slack, st_counts, sub_slack, sub_counts):
    c = small_docs()
    assert all(v > 3 for v in c["seen"].values()), c["seen"]
    state = pack(c["R"], c["st"], st_slack, st_counts, np.random.default_rng(11))
    sub = pack(c["R"], c["sub"], sub_slack, sub_counts, np.random.default_rng(12))
    assert (state.counts is None) == (not st_slack and not st_counts)
    want = check_scatter(eng, torch, state, sub, c["idx"])
    ident = select_ref(state)
    assert (want.offsets[1:] != ident.offsets[1:]).any()


# ------------------------------------------------------- 2. scan chunk edges

def tiny_batches(seed, n_docs, n_sub):
    """State of 0- to 3-entry documents with one slack slot each, and a
    sub-batch replacing n_sub of them: the first and last document and the
    documents on either side of every scan chunk boundary among them."""
    rng = np.random.default_rng(seed)

    def make(n, lo):
        cnt = rng.integers(0, 4, n).astype(U32)
        off = np.zeros(n + 1, U32)
        np.cumsum(cnt + U32(1), out=off[1:])
        tot = int(off[-1])
        return AWSetBatch(2, off, np.arange(tot, dtype=U64) * U64(2) + U64(lo),
                          rng.integers(0, 2, tot, dtype=np.int64).astype(U32),
                          rng.integers(1, 2 ** 40, tot, dtype=np.int64).view(U64).copy(),
                          rng.integers(0, 99, 2 * n, dtype=np.int64).view(U64).copy(), counts=cnt)

    state, sub = make(n_docs, 0), make(n_sub, 1)
    must = {0, n_docs - 1}
    for b in range(K_SCAN, n_docs, K_SCAN):
        must.update((b - 1, b))
    rest = [d for d in rng.permutation(n_docs).tolist() if d not in must]
    idx = np.array((sorted(must) + rest)[:n_sub], U32)
    rng.shuffle(idx)
    return state, sub, idx


@pytest.mark.parametrize("n_docs", [K_SCAN - 1, K_SCAN, K_SCAN + 1, 2 * K_SCAN - 1, 2 * K_SCAN, 2 * K_SCAN + 1,
                                    3 * K_SCAN - 1, 3 * K_SCAN, 3 * K_SCAN + 1])
def test_scan_chunk_edges(eng, torch, n_docs):
    state, sub, idx = tiny_batches(9900 + n_docs, n_docs, 400)
    check_scatter(eng, torch, state, sub, idx)


def test_partials_scan_steps(eng, torch):
    """More partial sums than one step of the partials scan holds: 1,026 chunks of
    0- or 1-entry documents, the expectation computed with numpy alone."""
    n = K_PART * K_SCAN + K_SCAN + 1
    state, sub, idx, want = one_entry_case(9950, n, 4096)
    assert (n + K_SCAN - 1) // K_SCAN > K_PART and {0, n - 1} <= set(idx.tolist())
    out = scatter_on_device(eng, torch, state, sub, idx, total=int(want.offsets[-1]))
    eng.sync()
    assert_packed(out, want)


# ----------------------------------------------------- 3. gather chunk edges

def _edge_case():
    """(state docs, sub docs, idx) whose OUTPUT has: documents ending one before,
    exactly at and one after a gather chunk boundary; a replaced document of 5,000
    entries that starts on a boundary and spans three chunks; 1,500 empty
    documents in a row (more than kSctRun stages), every other one a replacement;
    then 2,000 documents of 2 to 5 entries that alternate between the two sources."""
    rng = random.Random(9960)
    C = K_GATHER
    out_sizes = [C - 1, 1, C + 1, C - 1, 5000]
    from_sub = [False, True, True, False, True]
    assert sum(out_sizes[:1]) == C - 1 and sum(out_sizes[:2]) == C and sum(out_sizes[:3]) == 2 * C + 1
    assert sum(out_sizes[:4]) == 3 * C and 5000 > 2 * C
    for i in range(1500):
        out_sizes.append(0)
        from_sub.append(i % 2 == 1)
    for i in range(2000):
        out_sizes.append(rng.randint(2, 5))
        from_sub.append(i % 2 == 1)
    st, sub, idx = [], [], []
    for d, (n, s) in enumerate(zip(out_sizes, from_sub)):
        if s:  # the state's version has another length
            st.append(_seq_doc(7 * d, 3 if n != 3 else 1))
            k, a, c, _ = _seq_doc(7 * d + 1, n)
            sub.append((k, a, c, [d + 1, 9]))
            idx.append(d)
        else:
            k, a, c, _ = _seq_doc(7 * d, n)
            st.append((k, a, c, [d + 1, 3]))
    order = list(range(len(idx)))
    rng.shuffle(order)
    return st, [sub[j] for j in order], np.array([idx[j] for j in order], U32)


@pytest.mark.parametrize("st_slack,sub_slack", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_gather_chunk_edges(eng, torch, st_slack, sub_slack):
    """Slack 0: documents start where the last ended, pairs at even source slots
    are read with 16 B loads; slack 1: source runs start at odd slots on that side
    (element by element)."""
    st, sub, idx = _edge_case()
    state = pack(2, st, slack=st_slack, garbage=np.random.default_rng(5))
    subb = pack(2, sub, slack=sub_slack, garbage=np.random.default_rng(6))
    want = check_scatter(eng, torch, state, subb, idx)
    assert int(want.offsets[4]) == 3 * K_GATHER and int(want.counts[4]) == 5000
    assert not want.counts[5:1505].any() and 1500 > K_RUN


# ------------------------------------------------------------------ 4. clocks

@pytest.mark.parametrize("R", [1, 3, 64])
def test_clock_widths(eng, torch, R):
    rng = random.Random(9970 + R)
    n = 300
    st = [_rand_doc(rng, R, rng.choice((0, 1, 5))) for _ in range(n)]
    idx = rng.sample(range(n), 150)
    sub = [_rand_doc(rng, R, rng.choice((0, 1, 5))) for _ in idx]
    want = check_scatter(eng, torch, pack(R, st), pack(R, sub, slack=1), np.array(idx, U32))
    assert (want.vv.reshape(n, R)[idx[0]] == np.array(sub[0][3], U64)).all()


# ---------------------------------------------------------------- 5. the loop

_loop = {}


def loop_case():
    """A config-2-like pair of 3,000 documents of which about 10 % differ, and the
    full exchange of the two by the C oracle."""
    if not _loop:
        rng = random.Random(9980)
        R, n = 2, 3000
        da, db = [], []
        for d in range(n):
            k, a, c, v = _rand_doc(rng, R, rng.randint(0, 40))
            da.append((k, a, c, v))
            if rng.random() >= 0.1:
                db.append((k, a, c, v))
                continue
            kind = rng.randrange(4)
            k, a, c, v = list(k), list(a), list(c), list(v)
            if kind == 0 or not k:  # another document altogether
                k, a, c, v = _rand_doc(rng, R, rng.randint(0, 40))
            elif kind == 1:  # one element fewer
                i = rng.randrange(len(k))
                del k[i], a[i], c[i]
            elif kind == 2:  # one element under another dot
                c[-1] += 1
            else:  # the clock alone
                v[rng.randrange(R)] += 1
            db.append((k, a, c, v))
        a, b = pack(R, da, 3, 1, np.random.default_rng(13)), pack(R, db, 0, 1)
        rc1, ab = oracle.join(a, b)
        rc2, ba = oracle.join(b, a)
        assert rc1 == 0 and rc2 == 0
        _loop.update(R=R, n=n, a=a, b=b, cmp=compare_ref(a, b), ab=select_ref(ab.as_batch()),
                     ba=select_ref(ba.as_batch()))
    return _loop


@pytest.mark.parametrize("extra", [0, 5])
def test_sparse_round_on_the_device(eng, torch, extra):
    """compare -> select x2 -> exchange -> scatter x2 with the worklist and n_work
    left on the device; extra 5: the sub-batches hold more documents than the
    worklist names, and *n_idx keeps their empty tail out of the scatter."""
    c = loop_case()
    dev = dev_of(torch)
    R, n = c["R"], c["n"]
    flags, _, work = c["cmp"]
    assert 200 < len(work) < 400
    n_out = len(work) + extra
    sa_want = select_ref(c["a"], work, n_idx=len(work), n_out=n_out)
    sb_want = select_ref(c["b"], work, n_idx=len(work), n_out=n_out)
    ad, bd = c["a"].to(dev), c["b"].to(dev)
    res = poisoned_cmp(torch, n)
    sa = poisoned_out(torch, n_out, R, int(sa_want.offsets[-1]))
    sb = poisoned_out(torch, n_out, R, int(sb_want.offsets[-1]))
    xab = OutBuffers(n_out, R, sa.slots + sb.slots, device=dev)
    xba = OutBuffers(n_out, R, sa.slots + sb.slots, device=dev)
    new_a = poisoned_out(torch, n, R, int(c["ab"].offsets[-1]) + 4)
    new_b = poisoned_out(torch, n, R, int(c["ba"].offsets[-1]) + 4)
    res2 = poisoned_cmp(torch, n)
    eng.compare_async(ad, bd, res, mask=15)
    eng.select_async(ad, sa, idx=res.worklist, n_idx=res.n_work)
    eng.select_async(bd, sb, idx=res.worklist, n_idx=res.n_work)
    eng.exchange_async(sa.as_batch(), sb.as_batch(), xab, xba)
    eng.scatter_async(ad, xab.as_batch(), res.worklist, new_a, n_idx=res.n_work)
    eng.scatter_async(bd, xba.as_batch(), res.worklist, new_b, n_idx=res.n_work)
    eng.compare_async(new_a.as_batch(), new_b.as_batch(), res2, mask=15)
    eng.sync()
    assert_cmp(read_cmp(res), c["cmp"])
    assert_packed(new_a, c["ab"])
    assert_packed(new_b, c["ba"])
    flags2, summary2, _ = read_cmp(res2)
    assert not (flags2 & KEYS).any() and int(summary2[0]) == 0
    assert not flags2[flags == 0].any()  # what compared equal still does


# --------------------------------------------------- 6. no index, no document

def test_no_index_is_the_identity_select(eng, torch):
    c = small_docs()
    state = pack(c["R"], c["st"], 3, 1, np.random.default_rng(11))
    sub = pack(c["R"], c["sub"], 0, 0)
    dev = dev_of(torch)
    want = select_ref(state)
    out = scatter_on_device(eng, torch, state, sub, c["idx"], n_idx=0, total=int(want.offsets[-1]))
    sel = poisoned_out(torch, state.n_docs, state.R, int(want.offsets[-1]) + 3)
    eng.select_async(state.to(dev), sel)
    eng.sync()
    assert_packed(out, want)
    a, b = host_out(out), host_out(sel)
    for f in ("offsets", "counts", "keys", "actors", "counters", "vv"):
        assert (getattr(a, f) == getattr(b, f)).all(), f


def test_no_documents(eng, torch):
    dev = dev_of(torch)
    z = lambda dt: torch.zeros(1, dtype=dt, device=dev)  # noqa: E731
    e = AWSetBatch(2, z(torch.int32), z(torch.int64), z(torch.int32), z(torch.int64), z(torch.int64))
    assert e.n_docs == 0
    out = poisoned_out(torch, 1, 2, 4)
    eng.scatter_async(e, e, dev_words(torch, [0]), out, out_slots=4)
    eng.sync()
    h = host_out(out)
    assert int(h.offsets[0]) == 0 and int(h.offsets[1]) == ONES32 and (h.keys == MAXK).all()
    assert int(h.counts[0]) == ONES32 and (h.vv == MAXK).all()
    # a sub-batch of no documents: the identity select
    st = batch_of(2, [([(1, 0, 1), (4, 1, 2)], [1, 2]), ([], [0, 0]), ([(3, 0, 1)], [1, 0])], slack=1)
    out = poisoned_out(torch, 3, 2, 5)
    eng.scatter_async(st.to(dev), e, dev_words(torch, [0]), out)
    eng.sync()
    assert_packed(out, select_ref(st))


# ------------------------------------------------------------------ 7. errors

def test_index_out_of_range(eng, torch):
    c = small_docs()
    state, sub = pack(c["R"], c["st"], 3, 1), pack(c["R"], c["sub"][:5], 0, 0)
    idx = np.array([4, state.n_docs, 6, ONES32, 8], U32)
    want = scatter_ref(state, sub, idx)
    assert want.doc(4) == sub.doc(0) and want.doc(6) == sub.doc(2) and want.doc(8) == sub.doc(4)
    out = scatter_on_device(eng, torch, state, sub, idx, total=int(want.offsets[-1]))
    assert _code(eng.sync) == crdtgpu.CRDT_E_INVALID
    assert_packed(out, want)
    eng.sync()  # cleared


def test_duplicate_index_lowest_j_wins(eng, torch):
    c = small_docs()
    state, sub = pack(c["R"], c["st"], 0, 0), pack(c["R"], c["sub"][:6], 1, 1)
    idx = np.array([5, 9, 5, 9, 2, 5], U32)
    want = scatter_ref(state, sub, idx)
    assert want.doc(5) == sub.doc(0) and want.doc(9) == sub.doc(1) and want.doc(2) == sub.doc(4)
    assert sub.doc(0) != sub.doc(2) and sub.doc(0) != sub.doc(5)
    for _ in range(3):  # the same on every run
        out = scatter_on_device(eng, torch, state, sub, idx, total=int(want.offsets[-1]))
        assert _code(eng.sync) == crdtgpu.CRDT_E_INVALID
        assert_packed(out, want)


def test_n_idx_above_the_sub_batch_is_clamped(eng, torch):
    c = small_docs()
    state, sub = pack(c["R"], c["st"], 3, 1), pack(c["R"], c["sub"][:8], 0, 0)
    idx = np.arange(10, 18, dtype=U32)
    want = scatter_ref(state, sub, idx, n_idx=20)
    assert want.doc(17) == sub.doc(7)
    out = scatter_on_device(eng, torch, state, sub, idx, n_idx=20, total=int(want.offsets[-1]))
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    assert_packed(out, want)


def test_total_above_out_slots(eng, torch):
    c = small_docs()
    state, sub = pack(c["R"], c["st"], 3, 1), pack(c["R"], c["sub"], 0, 1)
    want = scatter_ref(state, sub, c["idx"])
    total = int(want.offsets[-1])
    cut = total - 777
    out = scatter_on_device(eng, torch, state, sub, c["idx"], spare=0, out_slots=cut, total=total)
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    h = host_out(out)
    assert (h.keys[cut:total] == MAXK).all() and (h.counters[cut:total] == MAXK).all()
    assert (h.actors[cut:total] == ONES32).all()
    assert (h.keys[:cut] == want.keys[:cut]).all() and (h.actors[:cut] == want.actors[:cut]).all()
    assert (h.counters[:cut] == want.counters[:cut]).all()
    assert (h.offsets == want.offsets).all() and (h.counts == want.counts).all() and (h.vv == want.vv).all()


@pytest.mark.parametrize("side", ["state", "sub"])
def test_count_above_slots_is_clamped(eng, torch, side):
    state = batch_of(2, [([(1, 0, 1)], [1, 0]), ([(3, 0, 1)], [1, 0]), ([(9, 1, 4)], [0, 4])], slack=1)
    sub = batch_of(2, [([(2, 1, 1)], [1, 1]), ([(6, 1, 2)], [0, 2])], slack=1)
    idx = np.array([2, 0], U32)
    over, d = (state, 1) if side == "state" else (sub, 1)
    over.keys[int(over.offsets[d]) + 1] = 77  # the slack slot: live once the count says so
    over.counts[d] = 5
    want = scatter_ref(state, sub, idx)
    assert want.counts.tolist() == ([2, 1, 1] if side == "sub" else [1, 2, 1])
    out = scatter_on_device(eng, torch, state, sub, idx, total=int(want.offsets[-1]))
    assert _code(eng.sync) == crdtgpu.CRDT_E_CAPACITY
    assert_packed(out, want)
    eng.sync()


def test_argument_errors(eng, torch):
    """Every one of these is refused on the host: nothing is launched."""
    dev = dev_of(torch)
    st = batch_of(2, [([(1, 0, 1), (4, 1, 2)], [1, 2]), ([(3, 0, 1)], [1, 0])], slack=1).to(dev)
    sub = batch_of(2, [([(5, 0, 1)], [1, 0])], slack=1).to(dev)
    sub3 = batch_of(3, [([(5, 0, 1)], [1, 0, 0])], slack=1).to(dev)
    idx = dev_words(torch, [1])
    out = poisoned_out(torch, 2, 2, 8)
    lib, ctx, ref = abi.lib(), eng._ctx, ctypes.byref

    def call(cs, cb, ci, co):
        return lib.crdt_awset_scatter_async(ctx, ref(cs) if cs else None, ref(cb) if cb else None, ci, None, 8,
                                            ref(co) if co else None, None)

    p = idx.data_ptr()
    assert call(None, sub.c(), p, out.c()) == crdtgpu.CRDT_E_INVALID
    assert call(st.c(), None, p, out.c()) == crdtgpu.CRDT_E_INVALID
    assert call(st.c(), sub.c(), None, out.c()) == crdtgpu.CRDT_E_INVALID
    assert call(st.c(), sub.c(), p, None) == crdtgpu.CRDT_E_INVALID
    assert call(st.c(), sub3.c(), p, out.c()) == crdtgpu.CRDT_E_INVALID  # R
    cs, cb = st.c(), sub.c()
    cs.R = cb.R = 65
    assert call(cs, cb, p, out.c()) == crdtgpu.CRDT_E_INVALID
    for src in (st, sub):  # an out array starting where a source's array of the same kind starts
        for f in ("offsets", "counts", "keys", "actors", "counters", "vv"):
            co = out.c()
            setattr(co, f, getattr(src, f).data_ptr())
            assert call(st.c(), sub.c(), p, co) == crdtgpu.CRDT_E_INVALID, f
    eng.sync()
    h = host_out(out)
    assert (h.offsets == ONES32).all() and (h.counts == ONES32).all() and (h.keys == MAXK).all()
    eng.scatter_async(st, sub, idx, out)  # and the call still works
    eng.sync()
    assert_packed(out, scatter_ref(st.numpy(), sub.numpy(), np.array([1], U32)))


# ---------------------------------------------------------------- 8. plumbing

def test_ordered_after_an_exchange_on_another_stream(eng, torch):
    c = xchg_case()
    dev = dev_of(torch)
    n, R = c["n"], c["R"]
    o1 = OutBuffers(n, R, c["slots"], device=dev)
    o2 = OutBuffers(n, R, c["slots"], device=dev)
    for o in (o1, o2):
        for t in (o.offsets, o.counts, o.keys, o.actors, o.counters, o.vv):
            t.zero_()  # a scatter that ran before the exchange would see an empty sub-batch
    da, db = c["a"].to(dev), c["b"].to(dev)
    idx = np.arange(n - 1, -1, -2, dtype=U32)  # every other document, descending
    # the sub-batch is the exchange's output itself: sub document j = document j of out_ab
    want = scatter_ref(c["a"], c["ab"].as_batch(), idx, n_idx=len(idx))
    out = poisoned_out(torch, n, R, int(want.offsets[-1]) + 2)
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    eng.exchange_async(da, db, o1, o2, stream=sa)
    eng.scatter_async(da, o1.as_batch(), dev_words(torch, idx), out, n_idx=dev_words(torch, [len(idx)]), stream=sb)
    eng.sync(sb)
    assert_packed(out, want)


def fixed_slots(R, docs, cap):
    """docs: [(keys, actors, counters, vv)] at `cap` slots per document, whatever they hold."""
    m = len(docs)
    b = AWSetBatch(R, np.arange(m + 1, dtype=U32) * U32(cap), np.zeros(m * cap, U64), np.zeros(m * cap, U32),
                   np.zeros(m * cap, U64), np.zeros(m * R, U64), counts=np.zeros(m, U32))
    for d, (k, a, c, v) in enumerate(docs):
        o, n = d * cap, len(k)
        assert n <= cap
        b.keys[o:o + n], b.actors[o:o + n], b.counters[o:o + n] = (np.asarray(k, U64), np.asarray(a, U32),
                                                                    np.asarray(c, U64))
        b.vv[d * R:(d + 1) * R] = v
        b.counts[d] = n
    return b


def test_graph_capture(torch):
    """A scatter captured on a reserved context and replayed with the sub-batch,
    the index list and *n_idx changed in between equals the eager call; on an
    unreserved context the capture is refused with CRDT_E_WORKSPACE and launches
    nothing."""
    c = small_docs()
    R = c["R"]
    state = pack(R, c["st"], 3, 1, np.random.default_rng(11))
    n = state.n_docs
    assert n > 1024  # (a fresh context's workspace holds 1,024 documents)
    m = 300
    rng = random.Random(9990)
    cases = []
    for r in range(3):
        docs = [_rand_doc(rng, R, rng.randint(0, 20)) for _ in range(m)]
        sub = fixed_slots(R, docs, 20)  # 20 slots each: every replay fits the same layout
        idx = np.array(rng.sample(range(n), m), U32)
        n_idx = (m, 120, 0)[r]
        cases.append((sub, idx, n_idx, scatter_ref(state, sub, idx, n_idx)))
    slots = max(int(w.offsets[-1]) for _, _, _, w in cases) + 3
    dev = dev_of(torch)
    e = crdtgpu.Engine(0)
    try:
        sd = state.to(dev)
        subd = AWSetBatch(R, *(torch.zeros(max(len(x), 1), dtype=torch.int64 if x.dtype == U64 else torch.int32,
                                           device=dev)[:len(x)]
                               for x in (cases[0][0].offsets, cases[0][0].keys, cases[0][0].actors,
                                         cases[0][0].counters, cases[0][0].vv)),
                          counts=torch.zeros(m, dtype=torch.int32, device=dev))
        idxd = torch.zeros(m, dtype=torch.int32, device=dev)
        n_idxd = torch.zeros(1, dtype=torch.int32, device=dev)
        out = poisoned_out(torch, n, R, slots)
        g0 = torch.cuda.CUDAGraph()
        with pytest.raises(crdtgpu.CrdtError) as ei:
            with torch.cuda.graph(g0):
                e.scatter_async(sd, subd, idxd, out, n_idx=n_idxd, stream=torch.cuda.current_stream())
        assert ei.value.code == crdtgpu.CRDT_E_WORKSPACE
        torch.cuda.synchronize()
        h = host_out(out)
        assert (h.offsets == ONES32).all() and (h.counts == ONES32).all() and (h.keys == MAXK).all()
        e.reserve(n)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            e.scatter_async(sd, subd, idxd, out, n_idx=n_idxd, stream=torch.cuda.current_stream())
        for sub, idx, n_idx, want in cases + cases[:1]:
            assert (sub.offsets == cases[0][0].offsets).all()
            sub_dev = sub.to(dev)
            for f in ("offsets", "counts", "keys", "actors", "counters", "vv"):
                getattr(subd, f).copy_(getattr(sub_dev, f))
            idxd.copy_(dev_words(torch, idx))
            n_idxd.fill_(n_idx)
            for t in (out.offsets, out.counts, out.keys, out.actors, out.counters, out.vv):
                t.fill_(-1)
            g.replay()
            e.sync(torch.cuda.current_stream())
            assert_packed(out, want)
    finally:
        e.close()
